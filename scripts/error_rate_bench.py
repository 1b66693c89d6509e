"""Throughput of the edit-distance alignment (csrc/edit_align.hip) on the two shapes a scoring run meets:

    (a) 25 000 pairs, reference length uniform in [5, 60], the hypothesis a noisy copy   (a test set of short utterances)
    (b) 64 pairs of 2048 x 2048 over a two-symbol alphabet                             (hallucinated transcripts; all ties)

For each: the whole op (table upload + both launches; device events around `repeats` calls after a warm-up), the two
kernels apiece from torch.profiler's device events of one further call, in cells/s (cells = sum of R * H), and
functional.edit_align end to end (host packing, launches, the results' way back).  Beside them the plain-Python
restatement of the tests (tests/edit_align_reference.py) on the host: 200 pairs of (a) and one 400 x 400 pair.

    python scripts/error_rate_bench.py [--repeats 20]"""
import argparse
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import edit_align_reference as R  # noqa: E402
import touchnet_amd.functional as F  # noqa: E402
import touchnet_amd.library as L  # noqa: E402


def workload_a(rng, n=25000):
    refs, hyps = [], []
    for _ in range(n):
        ref = [rng.randrange(4000) for _ in range(rng.randint(5, 60))]
        hyp = []
        for t in ref:
            u = rng.random()
            if u < 0.05:
                continue
            hyp.append(rng.randrange(4000) if u < 0.10 else t)
            if rng.random() < 0.05:
                hyp.append(rng.randrange(4000))
        refs.append(ref)
        hyps.append(hyp)
    return refs, hyps


def workload_b(rng, n=64, size=2048):
    return ([[rng.randrange(2) for _ in range(size)] for _ in range(n)],
            [[rng.randrange(2) for _ in range(size)] for _ in range(n)])


def one_launch(refs, hyps, dev):
    """the op's arguments for the whole batch in one launch, as functional.edit_align builds them"""
    (order, desc), = F.edit_align_tables([len(r) for r in refs], [len(h) for h in hyps], workspace_bytes=1 << 30)
    flat = lambda seqs: torch.tensor([t for i in order for t in seqs[i]], dtype=torch.int32, device=dev)
    ws_words = int(desc[-1, 4]) + L.edit_align_ws_words(int(desc[-1, 1]), int(desc[-1, 3]))
    return flat(refs), flat(hyps), torch.from_numpy(desc), ws_words * 4


def kernel_times(args):
    """{kernel name: microseconds} of one call, from the profiler's device events"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        L.edit_align(*args)
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        us = float(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        if "edit_" in ev.name and "kernel" in ev.name and us > 0:
            name = "forward" if "forward" in ev.name else "backtrace"
            out[name] = out.get(name, 0.0) + us
    return out


def device(name, refs, hyps, repeats, dev):
    cells = sum(len(r) * len(h) for r, h in zip(refs, hyps))
    arcs_max = sum(len(r) + len(h) for r, h in zip(refs, hyps))
    args = one_launch(refs, hyps, dev)
    for _ in range(3):
        L.edit_align(*args[:3])
    torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(repeats):
        L.edit_align(*args[:3])
    end.record()
    torch.cuda.synchronize()
    op_ms = beg.elapsed_time(end) / repeats
    print(f"({name}) {len(refs)} pairs, {cells / 1e6:.2f} M cells, workspace {args[3] / 2 ** 20:.1f} MiB")
    print(f"({name}) op (upload + forward + backtrace + output allocation), mean of {repeats}: {op_ms:.3f} ms  "
          f"{cells / op_ms / 1e6:.2f} G cells/s")
    try:
        kt = kernel_times(args[:3])
    except Exception as e:                                  # noqa: BLE001
        kt = {}
        print(f"({name}) kernel split not measured: torch.profiler failed ({e!r})")
    if set(kt) == {"forward", "backtrace"}:
        print(f"({name}) forward kernel:   {kt['forward'] / 1e3:.3f} ms  {cells / kt['forward'] / 1e3:.2f} G cells/s")
        print(f"({name}) backtrace kernel: {kt['backtrace'] / 1e3:.3f} ms  {cells / kt['backtrace'] / 1e3:.2f} G cells/s "
              f"(at most {arcs_max / kt['backtrace']:.1f} M arcs/s)")
    else:
        print(f"({name}) kernel split not measured: the profiler returned {sorted(kt) or 'no device events'}")
    t = time.perf_counter()
    out = F.edit_align(refs, hyps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    print(f"({name}) functional.edit_align end to end (host packing + device + unpacking): {dt * 1e3:.1f} ms  "
          f"{cells / dt / 1e6:.2f} M cells/s")
    return out


def host(name, refs, hyps, got=None):
    cells = sum(len(r) * len(h) for r, h in zip(refs, hyps))
    t = time.perf_counter()
    want = [R.align(r, h) for r, h in zip(refs, hyps)]
    dt = time.perf_counter() - t
    print(f"({name}) plain-Python restatement on the host, {len(refs)} pairs, {cells / 1e6:.3f} M cells: {dt * 1e3:.1f} ms  "
          f"{cells / dt / 1e6:.2f} M cells/s")
    if got is not None:
        same = all(g[4].tolist() == w[0] and tuple(g[:4]) == w[1] for g, w in zip(got, want))
        print(f"({name}) device arcs and counts equal the restatement's on these pairs: {same}")
        assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda", 0)
    prop = torch.cuda.get_device_properties(0)
    print(f"{prop.name} ({prop.gcnArchName}, {prop.multi_processor_count} CUs), torch {torch.__version__}, "
          f"{time.strftime('%Y-%m-%d')}")
    rng = random.Random(2026)
    refs, hyps = workload_a(rng)
    out = device("a", refs, hyps, args.repeats, dev)
    host("a", refs[:200], hyps[:200], out[:200])
    refs, hyps = workload_b(rng)
    out = device("b", refs, hyps, args.repeats, dev)
    host("b", [refs[0][:400]], [hyps[0][:400]])
    c, s, i, d, ops = out[0]
    assert c + s + d == 2048 and c + s + i == 2048 and ops.size == c + s + i + d


if __name__ == "__main__":
    main()
