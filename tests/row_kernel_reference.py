"""Plain float64 restatements of the row kernels (csrc/norm_act.hip) and the optimizer kernels (csrc/optim.hip), and
the error budget their GPU tests hold the kernels to.  No GPU, no HIP: torch on the CPU only.

Inputs are the kernel's own inputs (already in the kernel's dtype T, or fp32 statistics the kernel reads), widened to
float64.  A restatement applies exactly the roundings to T that the kernel's comments document (`rnd`), at the points
they name, and no others; its LAST rounding — the store of the output — is left to the kernel and stands in the
budget instead.  What then separates kernel and restatement is fp32 evaluation noise, the output rounding, and at most
one flip of a restated interior rounding whose fp32 argument fell on the other side of a tie.

Every function returns `Ref`s:
  value  the float64 result before the output rounding
  scale  sum of the absolute values of the terms that form `value` (NOT the possibly cancelled result): what the
         fp32 allowance is relative to.  For column sums and sums of squares the terms are the per-row products.
  flip   what one flip of a restated interior rounding moves the output by (0 where there is none)
  flush  v_exp_f32 / v_rcp_f32 flush a denormal result: an intermediate FACTOR whose float64 value is below 2^-126
         (sigmoid below -87.3, e^{-x^2 / 2} beyond |x| = 13.2) may read as zero, which moves the output by that factor
         times what multiplies it (`_flush`).  Zero wherever the factor is normal or exactly 0 / 1 — at the largest
         finite value of T in particular, where the budget is the half ulp and the fp32 allowance alone.

budget = roundings x half an ulp of T  +  FP32_REL x scale  +  flip  +  flush  +  TINY
(TINY = 2^-126: an output below the smallest normal may itself be flushed.)  The half ulp is taken at |value| + the
other terms, the largest magnitude the kernel's unrounded result may have: an allowance that carries a result over a
power of two lands where T is twice as coarse (w x xhat = 1.9963 with xhat flipped one bf16 ulp up is 2.008 and
rounds to 2.0156).
tests/test_row_kernel_reference_cpu.py holds every restatement to torch.nn.functional / oracle.nn / torch.optim in
float64, which is what makes this file a reference and not a second copy of the kernels."""
import math
from collections import namedtuple

import torch

F64 = torch.float64
FP32_REL = 1e-5          # the project's fp32 allowance (docstring of tests/test_kernels_gpu.py)
TINY = 2.0 ** -126       # smallest normal of fp32 and of bf16
_MANT = {torch.bfloat16: 8, torch.float32: 24, torch.float64: 53}

Ref = namedtuple("Ref", ["value", "scale", "flip", "flush"])


def _ref(value, scale, flip=None, flush=None):
    z = torch.zeros_like(value)
    return Ref(value, scale, z if flip is None else flip, z if flush is None else flush)


def _flush(f):
    """|f| where the factor f is below the smallest normal (the hardware may hand back 0 for it), else 0"""
    return torch.where(f.abs() < TINY, f.abs(), torch.zeros_like(f))


def d(t):
    return None if t is None else t.detach().cpu().to(F64)


def rnd(x, dtype):
    """float64 -> T -> float64 the way the kernels get there: through fp32 (their arithmetic), then to T."""
    return x if dtype == F64 else x.to(torch.float32).to(dtype).to(F64)


def ulp(x, dtype):
    """spacing of T at |x| (at least that of the smallest normal)"""
    _, e = torch.frexp(x.abs().clamp_min(TINY))              # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - _MANT[dtype])


def budget(ref, dtype, roundings=1):
    other = FP32_REL * ref.scale + ref.flip + ref.flush + TINY
    return roundings * 0.5 * ulp(ref.value.abs() + other, dtype) + other


def check(got, ref, dtype, what, roundings=1):
    """Every element of `got` within the budget of `ref` (and finite); prints and returns the worst error as a multiple
    of the budget.  On failure: the count, the worst index, the value there, the reference and the budget."""
    g = d(got).reshape(ref.value.shape)
    assert bool(torch.isfinite(ref.value).all()), f"{what}: the reference itself is not finite"
    b = budget(ref, dtype, roundings)
    err = (g - ref.value).abs()
    ratio = torch.where(torch.isfinite(g), err / b, torch.full_like(err, math.inf))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    name = {torch.bfloat16: "bf16", torch.float32: "fp32", F64: "fp64"}[dtype]
    print(f"measured: {what} [{name}] worst error = {worst:.3f} x budget")
    bad = ~(ratio <= 1.0)
    if bool(bad.any()):
        i = int(ratio.flatten().argmax())
        idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(
            f"{what} [{name}]: {int(bad.sum())}/{bad.numel()} elements over budget; worst at {idx}: "
            f"got {float(g.flatten()[i])!r}, ref {float(ref.value.flatten()[i])!r}, "
            f"budget {float(b.flatten()[i]):.4g} (error {float(err.flatten()[i]):.4g})")
    return worst


# ------------------------------------------------------------------------------------------------------ norms
def _add_residual(x, res, dtype):
    x = d(x)
    if res is None:
        return x, None
    s = x + d(res)
    return rnd(s, dtype), _ref(s, x.abs() + d(res).abs())


def rmsnorm_fwd(x, res, w, eps, dtype):
    """h = T(x + res);  rstd = rsqrt(mean(h^2) + eps);  y = T(w * T(h * rstd)).  -> dict(h (None without res), rstd, y)"""
    h, h_ref = _add_residual(x, res, dtype)
    w = d(w)
    rstd = torch.rsqrt((h * h).mean(-1) + eps)
    prod = h * rstd[:, None]
    xhat = rnd(prod, dtype)
    y = w * xhat
    return dict(h=h_ref, rstd=_ref(rstd, rstd), y=_ref(y, y.abs(), flip=w.abs() * ulp(prod, dtype)))


def rmsnorm_bwd(dy, h, w, rstd, dres, dtype):
    """xhat = T(h * rstd) as the forward rounded it;  g = dy * w;  dh = rstd * (g - xhat * mean(g * xhat)) (+ dres);
    dw = column sum of dy * xhat.  `rstd` is the fp32 statistic the kernel reads: h * rstd is then the exact product of
    two fp32 numbers on both sides and xhat cannot flip.  -> dict(dh, dw)"""
    dy, h, w, rstd = d(dy), d(h), d(w), d(rstd)[:, None]
    xhat = rnd(h * rstd, dtype)
    g = dy * w
    dot = (g * xhat).mean(-1, keepdim=True)
    dot_abs = (g * xhat).abs().mean(-1, keepdim=True)
    dh = rstd * (g - xhat * dot)
    sc = rstd * (g.abs() + xhat.abs() * dot_abs)
    if dres is not None:
        dh, sc = dh + d(dres), sc + d(dres).abs()
    return dict(dh=_ref(dh, sc), dw=_ref((dy * xhat).sum(0), (dy * xhat).abs().sum(0)))


def layernorm_fwd(x, res, w, b, eps, dtype):
    """h = T(x + res);  y = T((h - mean) * rstd * w + b), two-pass variance.  -> dict(h, mean, rstd, y)"""
    h, h_ref = _add_residual(x, res, dtype)
    w, b = d(w), d(b)
    mean = h.mean(-1, keepdim=True)
    dev = h - mean
    var = (dev * dev).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    spread = h.abs() + mean.abs()                              # the terms of h - mean
    mean_ref = _ref(mean[:, 0], h.abs().mean(-1))
    # The two-pass variance sums (h - mean_k)^2 with the kernel's own mean_k = mean + delta: all terms positive, and delta
    # enters as delta^2 only (sum(h - mean) = 0).  So rstd is held to 1e-5 of ITSELF plus rstd / 2 x delta^2 / (var + eps)
    # at the largest delta the mean's budget allows — which E[h^2] - mean^2 in fp32 cannot meet once |mean| >> spread.
    delta = budget(mean_ref, torch.float32)[:, None]
    rstd_ref = _ref(rstd[:, 0], rstd[:, 0], flip=(0.5 * rstd * delta * delta / (var + eps))[:, 0])
    y = dev * rstd * w + b
    return dict(h=h_ref, mean=mean_ref, rstd=rstd_ref, y=_ref(y, spread * rstd * w.abs() + b.abs()))


def layernorm_bwd(dy, h, w, mean, rstd, dres, dtype):
    """xhat = (h - mean) * rstd, unrounded;  g = dy * w;  dh = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ dres);
    dw = column sum of dy * xhat;  db = column sum of dy.  `mean`, `rstd`: the fp32 statistics the kernel reads."""
    dy, h, w, mean, rstd = d(dy), d(h), d(w), d(mean)[:, None], d(rstd)[:, None]
    xhat = (h - mean) * rstd
    g = dy * w
    s1, s2 = g.mean(-1, keepdim=True), (g * xhat).mean(-1, keepdim=True)
    a1, a2 = g.abs().mean(-1, keepdim=True), (g * xhat).abs().mean(-1, keepdim=True)
    dh = rstd * (g - s1 - xhat * s2)
    sc = rstd * (g.abs() + a1 + xhat.abs() * a2)
    if dres is not None:
        dh, sc = dh + d(dres), sc + d(dres).abs()
    return dict(dh=_ref(dh, sc), dw=_ref((dy * xhat).sum(0), (dy * xhat).abs().sum(0)),
                db=_ref(dy.sum(0), dy.abs().sum(0)))


# ------------------------------------------------------------------------------------------------------ activations
def swiglu_fwd(gate, up, dtype):
    """T(T(silu(gate)) * up)"""
    g, u = d(gate), d(up)
    s = torch.sigmoid(g)
    silu = g * s
    out = rnd(silu, dtype) * u
    return _ref(out, out.abs(), flip=u.abs() * ulp(silu, dtype), flush=u.abs() * (g.abs() * _flush(s) + _flush(silu)))


def swiglu_bwd(dout, gate, up, dtype):
    """d_up = T(dout * silu(g));  d_gate = T(dout * up * (s + silu(g) * (1 - s))), s = sigmoid(g); silu unrounded here.
    -> (d_gate, d_up)"""
    do, g, u = d(dout), d(gate), d(up)
    s = torch.sigmoid(g)
    silu = g * s
    lost = g.abs() * _flush(s) + _flush(silu)                  # what silu may lose to a flushed sigmoid / a flushed silu
    dg = do * u * (s + silu * (1 - s))
    return (_ref(dg, (do * u).abs() * (s + silu.abs() * (1 - s)), flush=(do * u).abs() * (_flush(s) + lost)),
            _ref(do * silu, (do * silu).abs(), flush=do.abs() * lost))


def _erf_parts(x):
    erf = torch.special.erf(x / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return erf, pdf


def _gelu_lost(x, cdf):
    """what the cdf may lose: the kernels form its lower tail as (at most half of) e^{-x^2 / 2}, and either may be flushed"""
    return _flush(cdf) + 0.5 * _flush(torch.exp(-0.5 * x * x))


def gelu_fwd(x):
    """x * (1 + erf(x / sqrt 2)) / 2 with the exact erf.  (The lower tail is taken from erfc: 1 + erf cancels there.)"""
    x = d(x)
    erf, _ = _erf_parts(x)
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    return _ref(x * cdf, x.abs() * (1 + erf.abs()) / 2, flush=x.abs() * _gelu_lost(x, cdf))


def gelu_bwd(dout, x):
    """dout * (cdf(x) + x * pdf(x))"""
    do, x = d(dout), d(x)
    erf, pdf = _erf_parts(x)
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    return _ref(do * (cdf + x * pdf), do.abs() * ((1 + erf.abs()) / 2 + x.abs() * pdf),
                flush=do.abs() * (_gelu_lost(x, cdf) + x.abs() * _flush(torch.exp(-0.5 * x * x))))


# ------------------------------------------------------------------------------------------------------ RoPE
ROPE_TABLE_ABS = 2e-6    # sincosf of an fp32 angle up to 2^24: absolute error of the fp32 table entries


def rope_table(pos, inv_freq, scaling):
    """cos / sin [n, half] of the fp32 product float(pos) * inv_freq (as the kernel forms it), taken in float64, times
    `scaling`.  -> (cos, sin) Refs whose flip field carries ROPE_TABLE_ABS."""
    ang = (pos.detach().cpu().to(torch.float32)[:, None] * inv_freq.detach().cpu().to(torch.float32)[None, :]).to(F64)
    sc = float(torch.tensor(scaling, dtype=torch.float32))
    c, s = torch.cos(ang) * sc, torch.sin(ang) * sc
    flat = torch.full_like(c, ROPE_TABLE_ABS)
    z = torch.zeros_like(c)
    return Ref(c, z, flat, z), Ref(s, z, flat, z)


def rope_apply(x, cos, sin, backward=False):
    """x [n, heads, D], cos / sin [n, D/2] (already in T): half-split rotation, for i < D/2
    y[i] = x[i] c[i] - x[i + D/2] s[i];  y[i + D/2] = x[i + D/2] c[i] + x[i] s[i];  `backward`: the transposed rotation."""
    x, c, s = d(x), d(cos)[:, None, :], d(sin)[:, None, :]
    if backward:
        s = -s
    half = x.shape[-1] // 2
    a, b = x[..., :half], x[..., half:]
    y = torch.cat((a * c - b * s, b * c + a * s), dim=-1)
    sc = torch.cat(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), dim=-1)
    return _ref(y, sc)


# ------------------------------------------------------------------------------------------------------ optimizer
def sumsq(g):
    g = d(g).flatten()
    s = (g * g).sum()
    return _ref(s, s)


def adamw_prepare(step, norm_sq, b1, b2, max_norm):
    """The device step state (adamw_prepare_kernel): the step advances on a finite norm only; bias corrections of the new
    step (of step 1 before the first applied step); clip = min(1, max_norm / (norm + 1e-6)), 1 without a norm, without
    a positive max_norm or on a skipped step.  `norm_sq` None = the entry's NULL.  -> (step, bc1, bc2, clip, skip)"""
    nsq = 0.0 if norm_sq is None else float(norm_sq)
    bad = not (math.isfinite(nsq) and nsq <= 3.0e38)
    step = step if bad else step + 1
    fs = max(step, 1)
    clip = 1.0
    if norm_sq is not None and max_norm > 0 and not bad:
        clip = min(1.0, max_norm / (math.sqrt(nsq) + 1e-6))
    return step, 1.0 - b1 ** fs, 1.0 - b2 ** fs, clip, bad


def adamw_step(p, m, v, g, step, lr, b1, b2, eps, wd, clip):
    """The rule of adamw_multi_kernel / adamw_kernel in float64.  -> (p, m, v, bf16 shadow of p)"""
    p, m, v, g = d(p), d(m), d(v), d(g) * clip
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v, p.to(torch.float32).to(torch.bfloat16)
