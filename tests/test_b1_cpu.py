"""CPU tests of binary points (packed bits under Hamming distance): the identity V0 = popcount(q xor r) that the
contract rests on, pack_bits' bit order and padding, the five entry points, and every answer the library gives before a
device is looked up (limits on k, alignment, flags, kn, radius, null pointers, sizes), plus the plan calls in words."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import v0_all  # noqa: E402

OK, INVALID, UNSUPPORTED = 0, 1, 5
B1 = 4   # the bf16_points / dtype value of binary points
SYMBOLS = ("nns_index_create_b1", "nns_index_search_b1", "nns_search_b1_ex", "nns_search_b1_topk", "nns_search_b1_range")
MAX_POINTS = 0x7FF00000   # NNS_MAX_POINTS


def _popcount_xor(qp, rp):
    """Hamming distances [m][n] of packed uint8 rows"""
    x = qp[:, None, :] ^ rp[None, :, :]
    return np.unpackbits(x, axis=2).sum(axis=2)


def test_the_five_b1_symbols_exist(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert getattr(raw, name) is not None
        assert name in pkg.ABI_SYMBOLS
    assert pkg.lib.nns_version() == 1


def test_v0_on_unpacked_bits_is_the_popcount_of_the_xor(pkg):
    rng = np.random.default_rng(1)
    for k in (32, 96, 1056):
        q = rng.integers(0, 2, (7, k)).astype(np.uint8)
        r = rng.integers(0, 2, (50, k)).astype(np.uint8)
        d = v0_all(q.astype(np.float32), r.astype(np.float32))
        want = _popcount_xor(pkg.pack_bits(q), pkg.pack_bits(r))
        assert np.array_equal(d, want.astype(np.float32)), k
        assert np.array_equal(d.astype(np.int64), (q[:, None, :] != r[None, :, :]).sum(axis=2)), k
    # all-zero against all-one rows: the largest distance at the largest k the tests use, every partial sum an integer
    k = 2048
    z, o = np.zeros((2, k), np.uint8), np.ones((3, k), np.uint8)
    assert (v0_all(z.astype(np.float32), o.astype(np.float32)) == np.float32(k)).all()
    assert (_popcount_xor(pkg.pack_bits(z), pkg.pack_bits(o)) == k).all()
    assert (v0_all(o.astype(np.float32), o.astype(np.float32)) == 0).all()
    assert 32 * 16384 < 2 ** 24   # the bound of the identity: the largest k keeps every sum exact in fp32


def test_pack_bits_bit_order_round_trip_and_padding(pkg):
    a = np.zeros((4, 64), np.uint8)
    a[0, 0] = 1      # bit 0 of word 0
    a[1, 31] = 1     # bit 31 of word 0
    a[2, 32] = 1     # bit 0 of word 1
    a[3, 63] = 1     # bit 31 of word 1
    p = pkg.pack_bits(a)
    assert p.dtype == np.uint8 and p.shape == (4, 8) and p.flags.c_contiguous
    w = p.view("<u4")
    assert w.tolist() == [[1, 0], [1 << 31, 0], [0, 1], [0, 1 << 31]]
    # bit t = (word[t / 32] >> (t % 32)) & 1, for random data; bool input gives the same bytes
    rng = np.random.default_rng(2)
    b = rng.integers(0, 2, (9, 96)).astype(np.uint8)
    wb = pkg.pack_bits(b).view("<u4")
    t = np.arange(96)
    assert np.array_equal((wb[:, t // 32] >> (t % 32).astype(np.uint32)) & 1, b)
    assert np.array_equal(pkg.pack_bits(b.astype(bool)), pkg.pack_bits(b))
    assert np.array_equal(np.unpackbits(pkg.pack_bits(b), axis=1, bitorder="little"), b)
    # k = 40 pads to 64 bits with zeros
    c = np.ones((3, 40), np.uint8)
    pc = pkg.pack_bits(c)
    assert pc.shape == (3, 8)
    assert np.array_equal(np.unpackbits(pc, axis=1, bitorder="little"), np.concatenate([c, np.zeros((3, 24), np.uint8)], 1))
    with pytest.raises(ValueError):
        pkg.pack_bits(np.array([[0, 2]]))
    with pytest.raises(ValueError):
        pkg.pack_bits(np.zeros(8, np.uint8))


def test_the_numpy_functions_take_packed_words_only(pkg):
    ok8 = np.zeros((4, 8), np.uint8)
    for fn, extra in ((pkg.search_b1, ()), (pkg.search_topk_b1, (2,)), (pkg.search_range_b1, (1.0,))):
        for bad in (np.zeros((4, 6), np.uint8), np.zeros((4, 8), np.int8), np.zeros((4, 2), np.float32),
                    np.zeros((4, 2), np.uint16), np.zeros(8, np.uint8)):
            with pytest.raises(ValueError):
                fn(bad, ok8, *extra)
            with pytest.raises(ValueError):
                fn(ok8, bad, *extra)
        with pytest.raises(ValueError):
            fn(ok8, np.zeros((4, 12), np.uint8), *extra)      # widths differ
    # uint32 words are the same points as their little-endian bytes
    w = np.array([[1, 1 << 31]], "<u4")
    assert np.array_equal(pkg.to_b1(w), w.view(np.uint8))
    buf = np.zeros(4 * 8 + 8, np.uint8)
    off = (-buf.ctypes.data) % 4                              # the first 4-byte aligned byte of buf
    assert pkg.to_b1(buf[off + 4:off + 36].reshape(4, 8)).ctypes.data % 4 == 0
    with pytest.raises(ValueError):
        pkg.to_b1(buf[off + 1:off + 33].reshape(4, 8))        # not 4-byte aligned


class _Calls:
    """the create call and the three whole calls on device 99 (no such device anywhere: a device lookup would answer
    NNS_ERR_NODEVICE, or NNS_ERR_INVALID with another text)"""

    def __init__(self, pkg, kwords=2, rows=4):
        self.L = pkg.lib
        self.buf = np.zeros(rows * kwords * 4 + 16, np.uint8)
        base = self.buf.ctypes.data
        self.pp = base + (-base) % 16                       # 16-byte aligned words
        self.h = ctypes.c_void_p()
        self.idx = np.zeros((rows, 300), np.int32)
        self.lims = np.zeros(rows + 1, np.int64)
        self.pidx = ctypes.POINTER(ctypes.c_int)()

    def create(self, k=64, n=4, p=None, flags=0, out=True):
        return self.L.nns_index_create_b1(ctypes.byref(self.h) if out else None, 99, k, n, self.pp if p is None else p, 0,
                                          flags, None)

    def ex(self, k=64, m=4, n=4, q=None, r=None, flags=0, idx=True):
        return self.L.nns_search_b1_ex(k, m, n, self.pp if q is None else q, self.pp if r is None else r,
                                       self.idx.ctypes.data if idx else None, None, 1, flags, 99)

    def topk(self, k=64, m=4, n=4, q=None, r=None, kn=2, flags=0, idx=True):
        return self.L.nns_search_b1_topk(k, m, n, self.pp if q is None else q, self.pp if r is None else r, kn,
                                         self.idx.ctypes.data if idx else None, None, 1, flags, 99)

    def range(self, k=64, m=4, n=4, q=None, r=None, radius2=1.0, flags=0, lims=True, idx=True):
        return self.L.nns_search_b1_range(k, m, n, self.pp if q is None else q, self.pp if r is None else r, radius2,
                                          self.lims.ctypes.data if lims else None,
                                          ctypes.byref(self.pidx) if idx else None, None, flags, 99)

    def all(self):
        return {"create": self.create, "ex": self.ex, "topk": self.topk, "range": self.range}


def test_flags_are_answered_before_the_device_lookup(pkg):
    c = _Calls(pkg)
    for name, call in c.all().items():
        for flag in (pkg.NNS_PATH_MFMA, pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA, pkg.NNS_REFS_SOA, pkg.NNS_RECORDS_PER_REF):
            assert call(flags=flag) == UNSUPPORTED, (name, flag)
            assert b"binary points" in c.L.nns_last_error(), (name, c.L.nns_last_error())
        for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER):
            assert call(flags=flag) == INVALID, (name, flag)
            assert b"operand flags" in c.L.nns_last_error(), (name, c.L.nns_last_error())
        assert b"NNS_" not in c.L.nns_last_error()
        # what is accepted gets as far as the device lookup: not one of the two answers above
        for flag in (pkg.NNS_PATH_AUTO, pkg.NNS_PATH_EXACT, pkg.NNS_PROFILE):
            rc = call(flags=flag)
            assert rc != OK and b"binary points" not in c.L.nns_last_error() and b"operand flags" not in c.L.nns_last_error(), \
                (name, flag, rc, c.L.nns_last_error())
    assert not c.h and not c.pidx


def test_limits_on_k_and_alignment_before_the_device_lookup(pkg):
    c = _Calls(pkg)
    for name, call in c.all().items():
        assert call(k=40) == UNSUPPORTED, name
        assert b"multiple of 32" in c.L.nns_last_error(), (name, c.L.nns_last_error())
        assert call(k=32 * 16385) == UNSUPPORTED, name
        assert b"16384" in c.L.nns_last_error(), (name, c.L.nns_last_error())
        assert call(k=0) == INVALID and call(k=-32) == INVALID, name
    # a pointer offset by 2 bytes, on either side
    assert c.create(p=c.pp + 2) == INVALID and b"aligned" in c.L.nns_last_error()
    for call in (c.ex, c.topk, c.range):
        assert call(q=c.pp + 2) == INVALID and b"aligned" in c.L.nns_last_error()
        assert call(r=c.pp + 2) == INVALID and b"aligned" in c.L.nns_last_error()
    assert not c.h and not c.pidx


def test_kn_radius_null_pointers_and_sizes(pkg):
    c = _Calls(pkg)
    assert c.topk(kn=0) == INVALID and c.topk(kn=-1) == INVALID
    assert c.topk(kn=257) == UNSUPPORTED
    assert c.range(radius2=float("nan")) == INVALID and c.range(radius2=-1.0) == INVALID
    # null pointers
    assert c.create(out=False) == INVALID
    assert c.L.nns_index_create_b1(ctypes.byref(c.h), 99, 64, 4, None, 0, 0, None) == INVALID
    assert c.L.nns_index_search_b1(None, 4, c.pp, c.pp, None) == INVALID
    assert c.L.nns_search_b1_ex(64, 4, 4, None, c.pp, c.idx.ctypes.data, None, 1, 0, 99) == INVALID
    assert c.L.nns_search_b1_ex(64, 4, 4, c.pp, None, c.idx.ctypes.data, None, 1, 0, 99) == INVALID
    assert c.ex(idx=False) == INVALID and c.topk(idx=False) == INVALID
    assert c.L.nns_search_b1_topk(64, 4, 4, c.pp, None, 2, c.idx.ctypes.data, None, 1, 0, 99) == INVALID
    assert c.range(idx=False) == INVALID and c.range(lims=False) == INVALID
    assert c.L.nns_search_b1_range(64, 4, 4, None, c.pp, 1.0, c.lims.ctypes.data, ctypes.byref(c.pidx), None, 0, 99) == INVALID
    # non-positive and oversized point counts
    for call in (c.ex, c.topk, c.range):
        assert call(m=0) == INVALID and call(n=0) == INVALID and call(n=-3) == INVALID
        assert call(m=MAX_POINTS + 1) == INVALID and b"NNS_MAX_POINTS" in c.L.nns_last_error()
        assert call(n=MAX_POINTS + 1) == INVALID and b"NNS_MAX_POINTS" in c.L.nns_last_error()
    assert c.create(n=0) == INVALID
    assert c.create(n=MAX_POINTS + 1) == INVALID and b"NNS_MAX_POINTS" in c.L.nns_last_error()
    assert not c.h and not c.pidx


def test_plan_calls_count_words(pkg):
    # the LDS bytes at k = 8192 bits are those of 256 words of 4 bytes, not of 8192 elements
    for m, n, kn in ((70, 3000, 10), (4096, 1 << 20, 100)):
        assert pkg.plan_topk(8192, m, n, kn, bf16=B1) == pkg.plan_topk(256, m, n, kn, bf16=False)
        assert pkg.plan_topk(8192, m, n, kn, bf16=B1) != pkg.plan_topk(8192, m, n, kn, bf16=False)
        assert pkg.plan_range(8192, m, n, bf16=B1) == pkg.plan_range(256, m, n, bf16=False)
        assert pkg.plan_range(8192, m, n, bf16=B1)["lds_bytes"] < pkg.plan_range(8192, m, n, bf16=False)["lds_bytes"]
    # (the tile itself: 4 bytes per word and query on top of what a one-word point needs)
    p, p1 = pkg.plan_range(8192, 70, 3000, bf16=B1), pkg.plan_range(32, 70, 3000, bf16=B1)
    assert p["queries_per_wg"] == p1["queries_per_wg"]
    assert p["lds_bytes"] - p1["lds_bytes"] == p["queries_per_wg"] * 255 * 4
    # the word limit, not the element limit: 2^19 bits plan, 40 bits and 2^19 + 32 bits do not
    out = np.zeros(16, np.int32)
    L = pkg.lib
    assert L.nns_plan_topk(32 * 16384, 70, 3000, 10, B1, out.ctypes.data, 6) == OK
    assert L.nns_plan_range(32 * 16384, 70, 3000, B1, out.ctypes.data, 6) == OK
    assert L.nns_plan_topk(32 * 16385, 70, 3000, 10, B1, out.ctypes.data, 6) == UNSUPPORTED
    assert L.nns_plan_range(32 * 16385, 70, 3000, B1, out.ctypes.data, 6) == UNSUPPORTED
    assert L.nns_plan_topk(40, 70, 3000, 10, B1, out.ctypes.data, 6) == UNSUPPORTED
    assert L.nns_plan_range(40, 70, 3000, B1, out.ctypes.data, 6) == UNSUPPORTED
    assert L.nns_plan_topk(0, 70, 3000, 10, B1, out.ctypes.data, 6) == INVALID
    # no filter for binary points
    assert L.nns_plan_filter(256, 64, 2048, B1, 0, out.ctypes.data, 16) == UNSUPPORTED
    assert L.nns_plan_filter(256, 4096, 1 << 20, B1, pkg.NNS_RECORDS_PER_REF, out.ctypes.data, 16) == UNSUPPORTED
