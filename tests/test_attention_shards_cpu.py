"""The segment contract of the sequence-sharded attention entry points (include/touchnet_amd.h above tn_attn_fwd_seg,
csrc/attn_common.h seg_view): what must hold WITHOUT the device.  tn_attn_fwd_seg, tn_attn_fwd_seg_chunks and
tn_attn_bwd_seg check a segment list on the host and return -22 before anything is launched; the kernels trust the list
(they index the local buffers and the global K / V with it), so a list they cannot serve must never reach them.

Only refused calls are made here.  The addresses are host memory, never dereferenced by a refused call."""
import ctypes as C

import pytest

EINVAL = -22
ENTRIES = ["tn_attn_fwd_seg", "tn_attn_fwd_seg_chunks", "tn_attn_bwd_seg"]


@pytest.fixture(scope="module")
def seg_call():
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    raw = (C.c_char * 8192)()                                # (the closure keeps it alive)
    p = (C.addressof(raw) + 255) // 256 * 256

    def call(entry, segs, rpb, T=512, nseg=None, chunk_len=128, null_segs=False):
        """One call of `entry` with B = 2, Nh = 4, Nkv = 2, D = 128 and `segs` = (row0, rows, off) triples."""
        flat = [int(x) for seg in segs for x in seg]
        n = len(segs) if nseg is None else nseg
        arr = None if null_segs else (C.c_int * 9)(*(flat + [0] * (9 - len(flat))))
        if entry == "tn_attn_fwd_seg":
            r = lib.tn_attn_fwd_seg(p, p, p, p, p, p, p, 2, T, 4, 2, 128, 0.125, n, arr, rpb, None)
        elif entry == "tn_attn_fwd_seg_chunks":
            r = lib.tn_attn_fwd_seg_chunks(p, p, p, p, p, p, p, 2, T, 4, 2, 128, 0.125, n, arr, rpb, chunk_len, 1, None)
        else:
            r = lib.tn_attn_bwd_seg(p, p, p, p, p, p, p, p, p, p, p, p, 2, T, 4, 2, 128, 0.125, n, arr, rpb, None)
        return r
    return call


# (segments, rows_per_batch, T) of every way a description can be unservable
REFUSED = {
    "rows_per_batch is zero": ([(0, 256, 0)], 0, 512),
    "rows_per_batch is negative": ([(0, 256, 0)], -256, 512),
    "a segment without rows": ([(0, 0, 0)], 256, 512),
    "a second segment without rows": ([(0, 128, 0), (128, 0, 256)], 256, 512),
    "a segment with negative rows": ([(0, -128, 128)], 256, 512),
    "a negative global offset": ([(0, 128, -128)], 256, 512),
    "a negative local row": ([(-128, 128, 0)], 256, 512),
    "a second segment at a negative local row": ([(0, 128, 0), (-128, 128, 256)], 256, 512),
    "a segment that ends behind T": ([(0, 256, 384)], 256, 512),
    "a segment that ends one position behind a ragged T": ([(0, 189, 512)], 256, 700),
    "a segment that starts at T": ([(0, 128, 512)], 256, 512),
    "a second segment that ends behind T": ([(0, 128, 0), (128, 256, 384)], 384, 512),
    "off + rows past INT_MAX": ([(0, 2 ** 31 - 1, 128)], 2 ** 31 - 1, 512),
    "a segment that ends behind the local buffer": ([(0, 256, 0)], 255, 512),
    "a segment at an offset that ends behind the local buffer": ([(128, 256, 0)], 256, 512),
    "a second segment that ends behind the local buffer": ([(0, 128, 0), (128, 200, 256)], 300, 512),
    "local ranges that overlap": ([(0, 256, 0), (128, 128, 256)], 256, 512),
    "the same local rows twice": ([(0, 128, 0), (0, 128, 256)], 256, 512),
    "local ranges that overlap, second segment first": ([(128, 128, 256), (0, 256, 0)], 256, 512),
    "global ranges that overlap": ([(0, 256, 0), (256, 128, 128)], 384, 512),
    "the same global positions twice": ([(0, 128, 128), (128, 128, 128)], 256, 512),
    "global ranges that overlap, descending": ([(0, 128, 128), (128, 256, 0)], 384, 512),
    # the rules the entry points had before
    "an offset that is no multiple of 128": ([(0, 128, 64)], 128, 512),
    "a second offset that is no multiple of 128": ([(0, 128, 0), (128, 128, 320)], 256, 512),
    "a local row that is no multiple of 128": ([(64, 128, 0)], 256, 512),
    "a second local row that is no multiple of 128": ([(0, 128, 0), (192, 128, 256)], 320, 512),
    "a ragged segment that is not the last": ([(0, 100, 0), (128, 128, 256)], 256, 512),
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_segment_descriptions_that_cannot_be_served_are_refused_before_any_launch(seg_call, entry):
    for what, (segs, rpb, T) in REFUSED.items():
        assert seg_call(entry, segs, rpb, T=T) == EINVAL, what


@pytest.mark.parametrize("entry", ENTRIES)
def test_segment_count_and_missing_list_are_refused(seg_call, entry):
    good = [(0, 128, 0), (128, 128, 256), (256, 128, 384)]
    assert seg_call(entry, good[:1], 384, null_segs=True) == EINVAL, "segs == nullptr"
    assert seg_call(entry, good[:2], 384, null_segs=True) == EINVAL, "segs == nullptr, two segments"
    assert seg_call(entry, good, 384, nseg=0) == EINVAL
    assert seg_call(entry, good, 384, nseg=3) == EINVAL
    assert seg_call(entry, good, 384, nseg=-1) == EINVAL


def test_chunk_restriction_rules_are_refused(seg_call):
    """chunk_len a positive multiple of 64, at most 64 chunks over T — for a segment list that is itself legal."""
    entry, segs = "tn_attn_fwd_seg_chunks", [(0, 256, 0)]
    assert seg_call(entry, segs, 256, chunk_len=96) == EINVAL
    assert seg_call(entry, segs, 256, chunk_len=100) == EINVAL
    assert seg_call(entry, segs, 256, chunk_len=0) == EINVAL
    assert seg_call(entry, segs, 256, chunk_len=-64) == EINVAL
    assert seg_call(entry, segs, 256, T=65 * 64, chunk_len=64) == EINVAL          # 65 chunks
    assert seg_call(entry, segs, 256, T=64 * 128 + 1, chunk_len=128) == EINVAL    # 64 whole chunks and one position
