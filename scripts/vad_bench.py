"""tn_vad_log_energy and tn_vad_runs (csrc/vad.hip) on int16 clips of 30 s, 10 min and 1 h at 16 kHz, 25 / 10 ms frames:
us per call of each entry, the clip's bytes at the device-copy rate measured in the same run (a device-to-device copy of a
buffer of the clip's size, read + write counted), and the plain torch composition of the log-energy as baseline
(unfold -> centred sum of squares -> log; it materialises the frames, 2.5x the clip, in fp32).

Raw C-ABI calls into buffers allocated once (no allocator in the timed region), HIP events around CALLS back-to-back
calls per round, the variants alternating round by round; median and min .. max over the rounds.

    python scripts/vad_bench.py [--rounds 9] [--log profiles/vad_bench.log]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, WIN, SHIFT = 16000, 400, 160
FLT_EPSILON = float(np.finfo(np.float32).eps)


def clip(seconds, seed=0):
    """int16 noise floor (sigma 30) with one tone burst in every four seconds"""
    g = torch.Generator().manual_seed(seed)
    n = seconds * SR
    x = torch.randn(n, generator=g) * 30.0
    t = torch.arange(n, dtype=torch.float32)
    x += 4000.0 * torch.sin(2 * np.pi * 440.0 * t / SR) * ((t / SR) % 4.0 < 1.5)
    return x.round().clamp(-32768, 32767).to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    from touchnet_amd import _C
    lib = _C.lib()
    dev = torch.device("cuda", 0)
    st = _C.stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; int16 clips at {SR} Hz, frames {WIN} / {SHIFT}; {args.rounds} rounds, us per call: "
        f"median (min .. max)")
    for seconds, calls in ((30, 200), (600, 50), (3600, 10)):
        pcm = clip(seconds).to(dev)
        N = pcm.numel()
        T = 1 + (N - WIN) // SHIFT
        fpb = lib.tn_vad_frames_per_block(WIN, SHIFT)
        loge = torch.empty(T, device=dev)
        partials = torch.empty(-(-T // fpb), dtype=torch.float64, device=dev)
        voiced = torch.empty(T, dtype=torch.uint8, device=dev)
        cap = T // 2 + 1
        buf = torch.empty(1 + 2 * cap, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.tn_vad_runs_workspace_bytes(T) // 8, dtype=torch.float64, device=dev)
        copy_dst = torch.empty_like(pcm)
        wave = pcm.float()                                # the baseline starts from fp32 on the int16 scale, conversion untimed

        def energy():
            assert lib.tn_vad_log_energy(p(pcm), 1, p(loge), p(partials), N, WIN, SHIFT, st) == 0

        def runs():
            assert lib.tn_vad_runs(p(loge), T, p(partials), partials.numel(), 5.0, 0.5, 0, 0.6, p(voiced),
                                   C.c_void_p(buf.data_ptr() + 4), p(buf), cap, p(ws), st) == 0

        def copy():
            copy_dst.copy_(pcm)

        def plain():
            f = wave.unfold(0, WIN, SHIFT)
            d = f - f.mean(dim=1, keepdim=True)
            return torch.log((d * d).sum(dim=1).clamp_min(FLT_EPSILON))

        variants = [("tn_vad_log_energy", energy, calls), ("tn_vad_runs (4 launches)", runs, calls),
                    ("device copy of the clip", copy, calls), ("torch unfold / centre / square / log", plain, max(calls // 10, 2))]
        for _, fn, _ in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        err = float((plain() - loge).abs().max())
        ts = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, fn, k in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(k):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ts[name].append(a.elapsed_time(b) * 1e3 / k)
        n_runs = int(buf[0])
        copy_us = statistics.median(ts["device copy of the clip"])
        rate = 2 * pcm.numel() * 2 / (copy_us * 1e-6)                     # bytes read + written per second
        nbytes = 2 * N + 4 * T
        say(f"{seconds} s: {N} samples, {T} frames, {n_runs} runs; max |loge - torch's| {err:.2e}; copy rate {rate / 1e12:.2f} "
            f"TB/s; the kernel's bytes ({nbytes / 1e6:.2f} MB: samples in, loge out) at that rate = {nbytes / rate * 1e6:.2f} us")
        for name, _, _ in variants:
            v = ts[name]
            say(f"    {name:40s} {statistics.median(v):10.2f} ({min(v):.2f} .. {max(v):.2f})")
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
