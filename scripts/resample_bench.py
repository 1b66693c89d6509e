"""tn_resample_sinc on 30 s clips of int16 PCM at 8 / 44.1 / 48 kHz -> 16 kHz: us per call, and the clip's bytes at the
6.3 TB/s copy rate.  (The logs under profiles/ also carry the column of the plain global-memory kernel that was timed
beside it, round by round, before it was deleted.)

Raw C-ABI calls into buffers allocated once (no allocator in the timed region), HIP events around CALLS back-to-back
calls per round; median and min .. max over the rounds.

    python scripts/resample_bench.py [--rounds 15] [--calls 200]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY = 6.3e12          # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--seconds", type=int, default=30)
    args = ap.parse_args()
    from touchnet_amd import _C
    import touchnet_amd.functional as F
    lib = _C.lib()
    dev = torch.device("cuda", 0)
    st = _C.stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    print(f"{torch.cuda.get_device_name(0)}; {args.seconds} s clips, int16 source; {args.rounds} rounds x {args.calls} calls, "
          f"us per call: median (min .. max)")
    for rate in (8000, 44100, 48000):
        o, n, ntap, tab = F.sinc_resample_table(rate, 16000)
        tab = torch.from_numpy(tab.astype(np.float32)).to(dev)
        N = args.seconds * rate
        n_out = -((-N * n) // o)
        g = torch.Generator().manual_seed(rate)
        pcm = torch.randint(-32768, 32768, (N,), generator=g, dtype=torch.int32).to(torch.int16).to(dev)
        y = torch.empty(n_out, device=dev)

        def sinc():
            assert lib.tn_resample_sinc(p(pcm), 1, p(y), p(tab), N, n_out, rate, 16000, ntap, st) == 0
        for _ in range(20):
            sinc()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                sinc()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / args.calls)
        nbytes = 2 * N + 4 * n_out
        print(f"{rate} -> 16000: {N} samples in, {n_out} out, {n} phases x {ntap} taps; "
              f"{nbytes / 1e6:.2f} MB at 6.3 TB/s = {nbytes / HBM_COPY * 1e6:.2f} us")
        print(f"    {'tn_resample_sinc':36s} {statistics.median(ts):8.2f} ({min(ts):.2f} .. {max(ts):.2f})")


if __name__ == "__main__":
    main()
