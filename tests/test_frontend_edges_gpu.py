"""tn_log_mel, tn_audiofeat_stack, tn_feat_augment and tn_bestrq_tokenize on the MI355X at their edges: the named cases of
tests/frontend_reference.py through touchnet_amd.functional, each run twice (identical bits), against the float64
restatements under the derived budgets — log-mel and the normalised stack per element, the plain stack, the augmentation
and the BEST-RQ codes exactly, on every row with none left out (test_frontend_reference_cpu.py has shown every margin
above ten times the fp32 error of a distance).

Measured on the MI355X (worst |kernel - float64| as a multiple of its budget, and the case):
  log-mel   0.035 of the budget on tone-1121 and tone-16077 at 80 bins (error 2.3e-7 under a budget of 6.6e-6, frame 2, the
            tone's own mel bin); 0.012 - 0.034 on every other case; the budgets there lie between 1.5e-6 and 1.8e-5, the largest
            error anywhere is 9.2e-6 (tone_noise-320, under the clamp's edge); silence is -1.5 in every element
  stack     0.125 of the budget on s1x1-T33-F64 (error 4.3e-7 under 3.9e-6); 0.044 - 0.123 elsewhere; mean 1000 / std 1e-3:
            error 0.068 under a budget of 1.12 (0.091); constant rows exactly zero; n = 1 NaN on both sides
  augment   bit-equal on every plan; the six refusals raise
  BEST-RQ   every code of every case equal, the lowest index on every planted tie, 0 on the NaN and the inf frame
The figures equal the fp32 emulation's of test_frontend_reference_cpu.py to the digits shown.  140 tests, 4.7 s in all
(1.8 s of it the first launch).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_reference as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _f():
    import touchnet_amd.functional as F
    return F


def _twice(fn):
    """Two launches, identical bits; the first one's result on the host."""
    a, b = fn().cpu(), fn().cpu()
    bits = torch.int64 if a.dtype == torch.int64 else torch.int32
    assert torch.equal(a.view(bits), b.view(bits)), "two launches differ"
    return a.numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================================================== log-mel
@pytest.mark.parametrize("n_mels", FR.LOG_MEL_BINS)
@pytest.mark.parametrize("name", sorted(FR.LOG_MEL_CASES))
def test_log_mel_stays_inside_the_derived_budget(name, n_mels):
    wav = FR.log_mel_wave(name)
    x = _dev(wav)
    got = _twice(lambda: _f().log_mel_spectrogram(x, n_mels))
    want, budget = FR.log_mel(wav, n_mels), FR.log_mel_budget(wav, n_mels)
    assert got.shape == want.shape == (wav.size // FR.HOP, n_mels)
    err = np.abs(got.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(err / budget), err.shape)
    print(f"log_mel {name} n_mels {n_mels}: {float((err / budget).max()):.3f} of the budget at {worst} "
          f"(error {err[worst]:.2e}, budget {budget[worst]:.2e}; largest error {err.max():.2e})")
    assert np.isfinite(got).all() and (err <= budget).all()
    if name.startswith("zeros"):
        assert (got == np.float32(-1.5)).all()


# ================================================================================================== stack
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("name", sorted(FR.STACK_CASES))
def test_stack_stays_inside_the_derived_budget(name, normalize):
    stack, stride, T, F, kind = FR.STACK_CASES[name]
    feat = FR.stack_input(name)
    x = _dev(feat)
    got = _twice(lambda: _f().audiofeat_stack(x, stack, stride, normalize))
    want = FR.stack(feat, stack, stride, normalize)
    assert got.shape == want.shape == (-(-T // stride), stack * F)
    if not normalize:
        assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(got.astype(np.float64), want)
        return
    if stack * F == 1:
        assert np.isnan(got).all() and np.isnan(want).all()
        return
    budget = FR.stack_budget(feat, stack, stride, True)
    err = np.abs(got.astype(np.float64) - want)
    print(f"stack {name}: {float((err / budget).max()):.3f} of the budget (largest error {err.max():.2e}, "
          f"largest budget {budget.max():.2e})")
    assert np.isfinite(got).all() and (err <= budget).all()
    if kind == "constant":
        assert (got == 0).all()


# ================================================================================================== augment
@pytest.mark.parametrize("name", sorted(FR.AUGMENT_CASES))
def test_augment_is_the_stage_chain_bit_for_bit(name):
    T, F, tm, fm, sb, rows = FR.AUGMENT_CASES[name]
    feat = FR.augment_input(T, F)
    x = _dev(feat)
    got = _twice(lambda: _f().feat_augment(x, tm, fm, sb, rows))
    want = FR.augment(feat, tm, fm, sb, rows)
    assert got.shape == want.shape and np.array_equal(got, want), name
    assert np.array_equal(x.cpu().numpy(), feat)                      # the input is read, never written


@pytest.mark.parametrize("name", sorted(FR.AUGMENT_REFUSALS))
def test_augment_refuses_what_the_plan_cannot_hold(name):
    from touchnet_amd import _C
    T, F, tm, fm, sb, rows = FR.AUGMENT_REFUSALS[name]
    x = _dev(FR.augment_input(T, F))
    with pytest.raises(_C.KernelError):
        _f().feat_augment(x, tm, fm, sb, rows)
    torch.cuda.synchronize()


# ================================================================================================== BEST-RQ
def _codes(c, feat=None):
    q, book = _dev(c["quantizer"]), _dev(c["codebook"])
    x = _dev(c["feat"] if feat is None else feat)
    return _twice(lambda: _f().bestrq_tokenize(x, q, book))


@pytest.mark.parametrize("name", sorted(FR.BESTRQ_CASES))
def test_bestrq_codes_equal_the_restatement_on_every_row(name):
    c = FR.bestrq_input(name)
    V = c["codebook"].shape[0]
    want, _ = FR.bestrq(c["feat"], c["quantizer"], c["codebook"])
    got = _codes(c)
    assert got.dtype == np.int64 and ((got >= 0) & (got < V)).all(), got
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0], got[got != want], want[got != want])
    plant = FR.BESTRQ_CASES[name]["plant"]
    if plant and plant[0] == "tie":
        assert got[0] == min(plant[1:])                               # the lowest index of the two copies
    if plant and plant[0] == "poison":
        clean = _codes(c, c["clean"])
        keep = np.arange(got.size) != FR.POISON_FRAME
        assert got[FR.POISON_FRAME] == 0 and np.array_equal(got[keep], clean[keep])
