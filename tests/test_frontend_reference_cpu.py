"""tests/frontend_reference.py can tell a right data-side kernel from a wrong one — shown without a device.

Each kernel's arithmetic is emulated in fp32 in the kernel's own accumulation order (fp32 fma = the float64 product and sum
rounded once): sequential fma over n for the 400-point DFT and over k for the mel sum; lane-strided partial sums and the
xor-butterfly for the stack; explicit differences, fma and sqrt, the per-thread scan, the lane butterfly and the wave
pass for BEST-RQ.  The correct emulation stays inside every budget on every case; every one-line mutant leaves it on the
case its test names.  The restatements themselves are held to torch (stft, argmin over norms) and to the oracle."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_reference as FR  # noqa: E402

f32, f64 = np.float32, np.float64


def fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ================================================================================================== log-mel
def _tables(symmetric=False):
    n = np.arange(FR.NFFT, dtype=f32)
    arg = (f32(2.0) * n / f32(FR.NFFT)).astype(f64)                  # the fp32 argument of sincospif
    c, s = np.cos(np.pi * arg).astype(f32), np.sin(np.pi * arg).astype(f32)
    cw = np.cos(np.pi * (f32(2.0) * n / f32(FR.NFFT - 1)).astype(f64)).astype(f32) if symmetric else c
    return c, s, f32(0.5) - f32(0.5) * cw


def emu_power(wav, mutant=None, fused=True):
    """The DFT stage of log_mel_kernel: fp32 [frames, 201]."""
    N = wav.size
    T = N // FR.HOP
    c, s, hann = _tables(symmetric=mutant == "symmetric_hann")
    t = np.arange(T) + (1 if mutant == "drop_first" else 0)
    src = t[:, None] * (FR.HOP + 1 if mutant == "hop" else FR.HOP) + np.arange(FR.NFFT)[None, :] - FR.NFFT // 2
    src = np.where(src < 0, -src, src)
    src = np.where(src >= N, (2 * N if mutant == "reflect" else 2 * (N - 1)) - src, src)
    ok = (src >= 0) & (src < N)
    xs = np.where(ok, wav[np.clip(src, 0, N - 1)], f32(0.0)).astype(f32) * hann[None, :]
    re = np.zeros((T, FR.NFREQ), f32)
    im = np.zeros((T, FR.NFREQ), f32)
    k = np.arange(FR.NFREQ)
    for n in range(FR.NFFT):
        idx = (n * k) % FR.NFFT
        x = xs[:, n:n + 1]
        if fused:
            re, im = fma(x, c[idx][None, :], re), fma(-x, s[idx][None, :], im)
        else:
            re, im = re + x * c[idx][None, :], im - x * s[idx][None, :]
    return fma(im, im, re * re)


def emu_finish(p, n_mels, mutant=None):
    """Mel sum, logarithm, global maximum and clamp of log_mel_kernel / log_mel_finish_kernel."""
    w = FR.slaney_filters(n_mels).astype(f32)
    acc = np.zeros((p.shape[0], n_mels), f32)
    for k in range(FR.NFREQ):
        acc = fma(w[None, :, k], p[:, k:k + 1], acc)
    v = np.log10(np.maximum(acc, f32(1e-10)).astype(f64)).astype(f32)
    gmax = v.max()
    if mutant == "negative_max_missed" and gmax < 0:
        gmax = f32(-np.inf)
    if mutant == "group_max":
        T = v.shape[0]
        pad = np.full((-T % FR.GROUP, n_mels), -np.inf, f32)
        g = np.concatenate([v, pad]).reshape(-1, FR.GROUP * n_mels).max(axis=1)
        gmax = np.repeat(g, FR.GROUP)[:T, None]
    return (np.maximum(v, gmax - f32(8.0)) + f32(4.0)) * f32(0.25)


@functools.lru_cache(maxsize=None)
def _power_of(name):
    wav = FR.log_mel_wave(name)
    return emu_power(wav, fused=wav.size < 100000)


def _log_mel_multiple(name, n_mels, got):
    wav = FR.log_mel_wave(name)
    return float((np.abs(got.astype(f64) - FR.log_mel(wav, n_mels)) / FR.log_mel_budget(wav, n_mels)).max())


def test_filters_window_and_frames_are_the_products_and_torchs():
    import touchnet_amd.functional as F
    for n_mels in FR.LOG_MEL_BINS:
        w = FR.slaney_filters(n_mels)
        assert w.shape == (n_mels, FR.NFREQ) and (w.sum(axis=1) > 0).all()
        got = F.slaney_mel_filters(n_mels, "cpu").numpy().astype(f64)
        assert (np.abs(got - w) <= 2 * FR.U * w + 1e-15).all()             # the fp32 table is this one rounded once
    for name in ("noise-201", "noise-399", "noise-799", "tone-1121"):
        wav = torch.from_numpy(FR.log_mel_wave(name)).double()
        st = torch.stft(wav, FR.NFFT, FR.HOP, window=torch.hann_window(FR.NFFT, dtype=torch.float64), return_complex=True)
        want = (st[..., :-1].abs() ** 2).T.numpy()
        assert np.allclose(FR.power(wav.numpy()), want, rtol=1e-10, atol=1e-12 * want.max())


@pytest.mark.parametrize("n_mels", FR.LOG_MEL_BINS)
@pytest.mark.parametrize("name", sorted(FR.LOG_MEL_CASES))
def test_log_mel_emulation_stays_inside_the_budget(name, n_mels):
    m = _log_mel_multiple(name, n_mels, emu_finish(_power_of(name), n_mels))
    print(f"{name} n_mels {n_mels}: emulation at {m:.3f} of the budget")
    assert m <= 1.0
    if name.startswith("zeros"):
        assert (emu_finish(_power_of(name), n_mels) == f32(-1.5)).all()
        assert (FR.log_mel(FR.log_mel_wave(name), n_mels) == -1.5).all()
    wav = FR.log_mel_wave(name).astype(f64)
    if name.startswith("quiet"):
        assert np.log10(np.maximum(FR.power(wav) @ FR.slaney_filters(n_mels).T, 1e-10)).max() < 0      # atomicMin branch


@pytest.mark.parametrize("mutant,name", [
    ("reflect", "noise-320"),               # right reflection 2 * n_samples - src: the last frame's mirrored half moves
    ("symmetric_hann", "tone-1121"),        # divide by 399: the on-bin tone leaks past its two neighbours, above the clamp
    ("drop_first", "noise-799"),            # frames 1 .. n instead of 0 .. n - 1
    ("hop", "noise-799"),                   # kHop 161
    ("group_max", "loud_last-long"),        # floor from each group's own maximum: the quiet groups sink below max - 8
    ("group_max", "loud_first-long"),
    ("negative_max_missed", "quiet_ends-1121"),   # maximum < 0 never recorded: the silent frames are not clamped
])
def test_a_wrong_log_mel_kernel_leaves_the_budget(mutant, name):
    """Right reflection `2 * n_samples - src` leaves the budget on noise-320, the symmetric Hann window on tone-1121, the
    first frame dropped and kHop = 161 on noise-799, the per-group maximum on loud_last-long and loud_first-long, the
    missed negative maximum on quiet_ends-1121.  Framing and window mutants are rerun from the waveform, clamp mutants
    from the correct power spectrum."""
    n_mels = 80
    if mutant in ("group_max", "negative_max_missed"):
        got = emu_finish(_power_of(name), n_mels, mutant)
    else:
        got = emu_finish(emu_power(FR.log_mel_wave(name), mutant), n_mels)
    m = _log_mel_multiple(name, n_mels, got)
    print(f"{mutant} on {name}: {m:.1f} of the budget")
    assert m > 1.0


def test_the_negative_maximum_alone_does_not_reach_the_clamp():
    """Why `quiet_ends` exists beside the issue's 1e-3 noise: below a maximum of -2 the floor max - 8 lies under
    log10(1e-10), so a lost negative maximum changes nothing there; only the device's atomicMin path is exercised."""
    name = "quiet-1121"
    assert np.array_equal(emu_finish(_power_of(name), 80, "negative_max_missed"), emu_finish(_power_of(name), 80))


# ================================================================================================== stack
def _butterfly_sum(s):
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, :1]


def emu_stack(x, stack, stride, normalize, mutant=None):
    """audiofeat_stack_kernel: one wave per row, lanes stride the row's n values."""
    T, F = x.shape
    n, rows = stack * F, -(-T // stride)
    lp = stack // 2 if mutant == "lp" else (stack - 1) // 2
    t = np.arange(rows)[:, None] * stride + np.arange(stack)[None, :] - lp
    xp = np.concatenate([x, np.full((1, F), 7.0, f32)])                      # what lies past the last row
    y = xp[np.clip(t, 0, T if mutant == "right_clamp" else T - 1)].reshape(rows, n)
    if not normalize:
        return y
    pad = -n % 64
    live = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(-1, 64)
    yl = np.concatenate([y, np.zeros((rows, pad), f32)], axis=1).reshape(rows, -1, 64)
    s = np.zeros((rows, 64), f32)
    for j in range(yl.shape[1]):
        s = s + yl[:, j, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = _butterfly_sum(s) / f32(n)
        ss = np.zeros((rows, 64), f32)
        for j in range(yl.shape[1]):
            d = yl[:, j, :] - mean
            ss = np.where(live[j][None, :], fma(d, d, ss), ss)
        var = _butterfly_sum(ss) / f32(n if mutant == "biased" else n - 1)
        inv = f32(1.0) / (np.sqrt(var + f32(1e-5)) if mutant == "eps_under_root" else np.sqrt(var) + f32(1e-5))
        return ((y - mean) * inv).astype(f32)


def _stack_multiple(name, normalize, got):
    stack, stride = FR.STACK_CASES[name][:2]
    x = FR.stack_input(name)
    want, budget = FR.stack(x, stack, stride, normalize), FR.stack_budget(x, stack, stride, normalize)
    err = np.abs(got.astype(f64) - want)
    if not normalize:
        return 0.0 if np.array_equal(got.astype(f64), want) else np.inf
    return float((err / budget).max())


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", sorted(FR.STACK_CASES))
def test_stack_emulation_stays_inside_the_budget(name, normalize):
    stack, stride, T, F, kind = FR.STACK_CASES[name]
    x = FR.stack_input(name)
    got = emu_stack(x, stack, stride, normalize)
    if normalize and stack * F == 1:
        assert np.isnan(got).all() and np.isnan(FR.stack(x, stack, stride, True)).all()
        return
    m = _stack_multiple(name, normalize, got)
    print(f"{name} normalize {normalize}: emulation at {m:.3f} of the budget")
    assert m <= 1.0
    if normalize and kind == "constant":
        assert (got == 0).all() and (FR.stack(x, stack, stride, True) == 0).all()


def test_stack_restatement_is_the_oracles_gather():
    import oracle.frontend as ofe
    for name in ("s4x4-T17-F140", "s7x6-T25-F80", "s5x4-T33-F112", "s7x1-T33-F80", "s1x1-T33-F64"):
        stack, stride = FR.STACK_CASES[name][:2]
        x = FR.stack_input(name)
        assert np.array_equal(ofe.audiofeat_stack(x, stack, stride, normalize=False), FR.stack(x, stack, stride, False))
        assert np.allclose(ofe.audiofeat_stack(x, stack, stride, normalize=True), FR.stack(x, stack, stride, True),
                           rtol=0, atol=1e-4)


@pytest.mark.parametrize("mutant,name,normalize", [
    ("lp", "s4x4-T17-F140", False),                 # lp = stack / 2: an even stack starts one frame early
    ("biased", "s5x4-T17-F13", True),               # / n: every value grows by 1 / (2 n) = 7.7e-3 of itself at n = 65
    ("right_clamp", "s7x6-T25-F80", False),         # clamp at T: the last row reads one row past the matrix
    ("eps_under_root", "small_std-s7x6-T25-F80", True),   # sqrt(var + 1e-5): 3.3e-3 against 1e-3 + 1e-5 at std 1e-3
])
def test_a_wrong_stack_kernel_leaves_the_budget(mutant, name, normalize):
    """`lp = stack / 2` differs on s4x4-T17-F140 and the right clamp at `T` on s7x6-T25-F80 (both plain gathers: any
    differing bit), the biased variance leaves the budget on s5x4-T17-F13, eps under the root on small_std-s7x6-T25-F80."""
    stack, stride = FR.STACK_CASES[name][:2]
    m = _stack_multiple(name, normalize, emu_stack(FR.stack_input(name), stack, stride, normalize, mutant))
    print(f"{mutant} on {name}: {m:.1f} of the budget")
    assert m > 1.0


# ================================================================================================== augment
def emu_augment(x, t_masks, f_masks, subs, out_rows, mutant=None):
    """feat_augment_kernel: one gather per output element."""
    T, F = x.shape
    incl = 1 if mutant == "end_inclusive" else 0
    t = np.arange(out_rows)
    src, done = t.copy(), np.zeros(out_rows, bool)
    order = range(len(subs)) if mutant == "first_wins" else range(len(subs) - 1, -1, -1)
    for k in order:
        s, e, pos = subs[k]
        hit = ~done & (t >= s) & (t < e + incl)
        src[hit] = t[hit] - pos
        done |= hit
    row = t if mutant == "dest_row" else src
    zt = np.zeros(out_rows, bool)
    for s, e in t_masks:
        zt |= (row >= s) & (row < e + incl)
    zf = np.zeros(F, bool)
    for s, e in f_masks:
        zf |= (np.arange(F) >= s) & (np.arange(F) < e + incl)
    return np.where(zt[:, None] | zf[None, :], f32(0.0), x[src])


@pytest.mark.parametrize("name", sorted(FR.AUGMENT_CASES))
def test_augment_emulation_is_the_stage_chain(name):
    T, F, tm, fm, sb, rows = FR.AUGMENT_CASES[name]
    assert len(tm) <= 16 and len(fm) <= 16 and len(sb) <= 16 and 1 <= rows <= T
    assert all(0 <= p <= s <= e <= T for s, e, p in sb)                      # what the entry point accepts
    x = FR.augment_input(T, F)
    want = FR.augment(x, tm, fm, sb, rows)
    assert want.shape == (rows, F) and want.dtype == np.float32
    assert np.array_equal(emu_augment(x, tm, fm, sb, rows), want)


def test_augment_restatement_is_the_oracles_stages():
    """The same draws through oracle.frontend's stage functions (the reference's random calls) and through the plan."""
    import random

    import oracle.frontend as ofe

    class Rec(random.Random):
        def __init__(self, seed):
            super().__init__(seed)
            self.out = []

        def randint(self, a, b):
            v = super().randint(a, b)
            self.out.append(v)
            return v
    x = FR.augment_input(300, 7)
    rng = Rec(5)
    y = ofe.spec_sub(ofe.spec_aug(x, 3, 2, 40, 3, rng), 3, 30, rng)
    d = rng.out
    tm = [(d[2 * k], min(300, d[2 * k] + d[2 * k + 1])) for k in range(3)]
    fm = [(d[6 + 2 * k], min(7, d[6 + 2 * k] + d[7 + 2 * k])) for k in range(2)]
    sb = [(d[10 + 3 * k], min(300, d[10 + 3 * k] + d[11 + 3 * k]), d[12 + 3 * k]) for k in range(3)]
    assert np.array_equal(np.asarray(y), FR.augment(x, tm, fm, sb, 300))


@pytest.mark.parametrize("mutant,name", [
    ("dest_row", "t300-f80-src-striped"),       # rows [40, 50) copy the zeroed rows [10, 20): the destination is clean
    ("dest_row", "t300-f80-dst-striped"),       # and rows [100, 110) receive clean rows although they lie in a stripe
    ("first_wins", "t300-f80-overlap-a"),       # rows [120, 130) belong to the later substitution
    ("first_wins", "t300-f80-overlap-b"),
    ("end_inclusive", "t1-f7-masked"),          # frequency stripe (2, 4) would also zero column 4
    ("end_inclusive", "t300-f80-src-striped"),  # time stripe (10, 20) would also zero row 20
])
def test_a_wrong_augment_kernel_differs(mutant, name):
    """The stripe tested on the destination row differs on t300-f80-src-striped and t300-f80-dst-striped, the first
    matching substitution on t300-f80-overlap-a and -b, the inclusive `end` on t1-f7-masked and t300-f80-src-striped."""
    T, F, tm, fm, sb, rows = FR.AUGMENT_CASES[name]
    x = FR.augment_input(T, F)
    assert not np.array_equal(emu_augment(x, tm, fm, sb, rows, mutant), FR.augment(x, tm, fm, sb, rows))


# ================================================================================================== BEST-RQ
SENTINEL = 0x7fffffff


def emu_bestrq(feat, q, book, mutant=None, fixed=True):
    """bestrq_tokenize_kernel.  The projection runs every 64-column chunk to its end over zero-filled tails — the same
    sums as the kernel's loop to min(64, F - k0), adding exact zeros — so the tail guard carries weight here."""
    T, F = feat.shape
    E, V = q.shape[1], book.shape[0]
    KC = 64
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((T, E), f32)
        ftile, qtile = np.full((T, KC), np.nan, f32), np.full((KC, E), np.nan, f32)     # LDS before the first store
        for k0 in range(0, F, KC):
            kn = min(KC, F - k0)
            if mutant != "tail_not_zeroed":
                ftile[:], qtile[:] = 0, 0
            ftile[:, :kn], qtile[:kn] = feat[:, k0:k0 + kn], q[k0:k0 + kn]
            for k in range(KC):
                acc = fma(ftile[:, k:k + 1], qtile[k][None, :], acc)
        s = np.zeros(T, f32)
        for e in range(E):
            s = fma(acc[:, e], acc[:, e], s)
        x = acc / np.maximum(np.sqrt(s), f32(1e-8))[:, None]
        codes = np.zeros(T, np.int64)
        lane = np.arange(64)
        for t0 in range(0, T, 32):
            xt = x[t0:t0 + 32]
            d2 = np.zeros((xt.shape[0], V), f32)
            for e in range(E):
                df = xt[:, e:e + 1] - book[None, :, e]
                d2 = fma(df, df, d2)
            d = np.sqrt(d2)
            # per-thread scan over v = tid, tid + 256, ...: `d < best` from (+inf, sentinel); NaN never wins
            d = np.where(np.isnan(d), f32(np.inf), d)
            dp = np.concatenate([d, np.full((d.shape[0], -V % 256), np.inf, f32)], axis=1).reshape(d.shape[0], -1, 256)
            J = dp.shape[1]
            j = (J - 1 - np.argmin(dp[:, ::-1, :], axis=1)) if mutant == "less_equal" else np.argmin(dp, axis=1)
            best = np.take_along_axis(dp, j[:, None, :], axis=1)[:, 0, :]
            idx = np.where(best < np.inf, j * 256 + np.arange(256)[None, :], SENTINEL)
            best, idx = best.reshape(-1, 4, 64), idx.reshape(-1, 4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                ob, oi = best[:, :, lane ^ o], idx[:, :, lane ^ o]
                take = (ob < best) if mutant == "index_ignored" else (ob < best) | ((ob == best) & (oi < idx))
                best, idx = np.where(take, ob, best), np.where(take, oi, idx)
            wb, wi = best[:, :, 0], idx[:, :, 0]
            b, i = wb[:, 0], wi[:, 0]
            for w in range(1, 4):
                take = (wb[:, w] < b) | ((wb[:, w] == b) & (wi[:, w] < i))
                b, i = np.where(take, wb[:, w], b), np.where(take, wi[:, w], i)
            codes[t0:t0 + 32] = np.where(i == SENTINEL, 0, i) if fixed else i
    return codes


FINITE = [n for n in sorted(FR.BESTRQ_CASES) if FR.BESTRQ_CASES[n]["plant"] is None or FR.BESTRQ_CASES[n]["plant"][0] != "poison"]
POISONED = [n for n in sorted(FR.BESTRQ_CASES) if n not in FINITE]


def test_bestrq_cases_cover_what_they_claim():
    ks = list(FR.BESTRQ_CASES.values())
    for E in (8, 16, 32):
        assert sum(k["E"] == E for k in ks) >= 2
    assert {1, 63, 256, 257, 300, 1024, 8192} <= {k["V"] for k in ks}
    assert {1, 24, 63, 64, 65, 560} <= {k["F"] for k in ks}
    assert {1, 31, 32, 33, 97} <= {k["T"] for k in ks}


@pytest.mark.parametrize("name", FINITE)
def test_bestrq_margins_clear_ten_bounds_and_the_emulation_agrees(name):
    """Every frame of every finite case keeps its best / second-best gap above ten times the fp32 error of a distance, so
    the device test may ask for equality on every row; the fp32 emulation and a float64 torch evaluation agree."""
    c = FR.bestrq_input(name)
    codes, margin = FR.bestrq(c["feat"], c["quantizer"], c["codebook"])
    bound = FR.bestrq_bound(c["feat"], c["quantizer"])
    ratio = float((margin / bound).min())
    print(f"{name}: smallest margin {margin.min():.2e}, largest bound {bound.max():.2e}, margin / bound >= {ratio:.1f}")
    assert np.isfinite(bound).all() and ratio > 10.0
    assert np.array_equal(emu_bestrq(c["feat"], c["quantizer"], c["codebook"]), codes)
    xs = torch.nn.functional.normalize(torch.from_numpy(c["feat"]).double() @ torch.from_numpy(c["quantizer"]).double(),
                                       dim=-1, p=2, eps=1e-8)
    want = torch.linalg.vector_norm(xs.unsqueeze(1) - torch.from_numpy(c["codebook"]).double().unsqueeze(0), dim=-1,
                                    ord=2).argmin(dim=-1).numpy()
    assert np.array_equal(want, codes)
    plant = FR.BESTRQ_CASES[name]["plant"]
    if plant and plant[0] == "tie":
        lo, hi = sorted(plant[1:])
        assert codes[0] == lo and np.array_equal(c["codebook"][lo], c["codebook"][hi])
    if plant and plant[0] == "tiny":
        assert codes[3] == codes[7] == int(np.argmin(np.linalg.norm(c["codebook"].astype(f64), axis=1)))


@pytest.mark.parametrize("name", POISONED)
def test_bestrq_non_finite_frame(name):
    """The poisoned frame gets code 0 and leaves the other 32 codes alone; without the final store's guard the kernel's
    arithmetic hands back its sentinel, 2147483647 — the defect this suite was written against."""
    c = FR.bestrq_input(name)
    codes, margin = FR.bestrq(c["feat"], c["quantizer"], c["codebook"])
    clean, clean_margin = FR.bestrq(c["clean"], c["quantizer"], c["codebook"])
    keep = np.arange(codes.size) != FR.POISON_FRAME
    assert codes[FR.POISON_FRAME] == 0 and np.array_equal(codes[keep], clean[keep])
    assert (clean_margin / FR.bestrq_bound(c["clean"], c["quantizer"])).min() > 10.0
    assert np.array_equal(emu_bestrq(c["feat"], c["quantizer"], c["codebook"]), codes)
    assert emu_bestrq(c["feat"], c["quantizer"], c["codebook"], fixed=False)[FR.POISON_FRAME] == SENTINEL


@pytest.mark.parametrize("mutant,name", [
    ("less_equal", "tie-same-thread-up-e16"),      # `<=`: thread 5 keeps row 261, its later copy
    ("less_equal", "tie-same-thread-e8"),
    ("index_ignored", "tie-next-lane-up-e16"),     # rows 71 / 72, lanes 7 / 8 of wave 1: lane 0's side holds 72 and keeps it
    ("tail_not_zeroed", "e16-v300-f65-t33"),       # chunk 2 has one live column; 63 stale ones are added again
])
def test_a_wrong_bestrq_kernel_changes_codes(mutant, name):
    """`<=` in the per-thread scan changes a code on tie-same-thread-up-e16 and tie-same-thread-e8, the index ignored in
    the lane reduction on tie-next-lane-up-e16, a chunk's tail columns left as they were on e16-v300-f65-t33."""
    c = FR.bestrq_input(name)
    codes, _ = FR.bestrq(c["feat"], c["quantizer"], c["codebook"])
    got = emu_bestrq(c["feat"], c["quantizer"], c["codebook"], mutant)
    print(f"{mutant} on {name}: {(got != codes).sum()} of {codes.size} codes differ")
    assert not np.array_equal(got, codes)
