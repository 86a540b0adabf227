"""GPU tests of top-K (k nearest neighbours, K6) against the numpy V0 oracle of test_topk_cpu.py: indices exact,
distances bit for bit, on the whole-call and split APIs, every path an index can be created for, fp32 and bf16
points, ties across split and shard boundaries, non-finite data, and the library's manners."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_topk_cpu import topk_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0x7F80000000000000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(idx, dist, want_idx, want_dist, what):
    bad = np.argwhere(idx != want_idx)
    assert bad.size == 0, f"{what}: {len(bad)} index mismatches, first at {bad[:3].tolist()}"
    assert np.array_equal(_bits(dist), _bits(want_dist)), f"{what}: distance bits differ"


def _check_whole(pkg, q, r, kn, **kw):
    want_idx, want_dist = topk_oracle(q, r, kn)
    idx, dist = pkg.search_topk(q, r, kn, return_distances=True, **kw)
    _assert_same(idx, dist, want_idx, want_dist, f"m={q.shape[0]} n={r.shape[0]} k={q.shape[1]} kn={kn} {kw}")
    return idx, dist


def _rand(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 16, 33, 128, 300])
def test_kn1_equals_nearest_neighbour(pkg, k):
    dev = torch.device("cuda:0")
    m, n = 200, 3000
    q = torch.from_numpy(_rand(100 + k, m, k)).to(dev)
    r = torch.from_numpy(_rand(200 + k, n, k)).to(dev)
    for path in ("auto", "exact", "mfma"):
        if path == "mfma" and k > 256:
            continue
        ix = pkg.Index(r, path=path, index_base=5)
        want = ix.search_keys(q)
        got = ix.search_topk_keys(q, 1)
        torch.cuda.synchronize()
        assert torch.equal(got[:, 0], want), (k, path)
        ix.close()


@pytest.mark.parametrize("k", [32, 256])
def test_kn1_equals_nearest_neighbour_bf16(pkg, k):
    dev = torch.device("cuda:0")
    m, n = 150, 2000
    q = torch.from_numpy(_rand(300 + k, m, k)).to(dev).to(torch.bfloat16)
    r = torch.from_numpy(_rand(400 + k, n, k)).to(dev).to(torch.bfloat16)
    for path in ("auto", "exact", "mfma"):
        ix = pkg.Index(r, path=path)
        want = ix.search_keys(q)
        got = ix.search_topk_keys(q, 1)
        torch.cuda.synchronize()
        assert torch.equal(got[:, 0], want), (k, path)
        ix.close()


# (k, m, n, kn): a sample of {1,3,5,16,33,128,257,1024} x {1,3,64,513} x {1,7,1000,70000} x {1,2,7,16,64,100,256}
# that keeps the oracle's m * n * k in reach of numpy
GRID = [
    (1, 1, 1, 1), (1, 513, 70000, 7), (1, 64, 1000, 256), (1, 3, 7, 16),
    (3, 1, 70000, 100), (3, 513, 1000, 64), (3, 64, 70000, 2), (3, 3, 7, 1),
    (5, 3, 70000, 256), (5, 513, 7, 7), (5, 64, 1000, 16), (5, 1, 1, 2),
    (16, 64, 70000, 100), (16, 513, 1000, 1), (16, 1, 70000, 256), (16, 3, 1000, 7),
    (33, 64, 1000, 64), (33, 3, 70000, 16), (33, 513, 7, 256), (33, 1, 1000, 2),
    (128, 3, 70000, 100), (128, 64, 1000, 7), (128, 513, 1000, 256), (128, 1, 7, 64),
    (257, 1, 70000, 16), (257, 64, 1000, 100), (257, 3, 1, 1),
    (1024, 3, 1000, 256), (1024, 64, 1000, 2), (1024, 1, 70000, 7),
]


@pytest.mark.parametrize("shape", GRID, ids=[f"k{k}-m{m}-n{n}-kn{kn}" for k, m, n, kn in GRID])
def test_random_grid_vs_oracle(pkg, shape):
    k, m, n, kn = shape
    seed = k * 7919 + m * 31 + n + kn
    q = _rand(seed, m, k)
    r = _rand(seed + 1, n, k)
    _check_whole(pkg, q, r, kn)


def test_many_copies_of_one_point(pkg):
    k, n = 16, 1000
    r = _rand(11, n, k)
    p = _rand(12, 1, k)[0]
    r[100:400] = p
    q = np.stack([p, _rand(13, k)])
    idx, _ = _check_whole(pkg, q, r, 256)
    assert idx[0].tolist() == list(range(100, 356))


def test_all_refs_equal(pkg):
    r = np.tile(_rand(14, 1, 7), (5000, 1))
    q = _rand(15, 9, 7)
    idx, _ = _check_whole(pkg, q, r, 100)
    assert (idx == np.arange(100)[None, :]).all()


def test_ties_across_split_and_shard_boundaries(pkg):
    k, n, kn = 3, 1 << 16, 16
    plan = pkg.plan_topk(k, 2, n, kn)
    assert plan["splits"] > 1
    b = plan["per"]                         # first split boundary
    r = _rand(16, n, k)
    p = np.array([5.0, 5.0, 5.0], np.float32)
    r[b - 5:b + 5] = p                      # equal distances on both sides of a split boundary
    r[n // 2 - 4:n // 2 + 4] = p            # ... and of the boundary of two shards
    q = np.stack([p, p + np.float32(0.25)])
    want_idx, _ = topk_oracle(q, r, kn)
    assert want_idx[0, :10].tolist() == list(range(b - 5, b + 5))
    for shards in (1, 2):
        _check_whole(pkg, q, r, kn, shards=shards)


def test_nonfinite_refs_are_never_returned(pkg):
    k, n = 4, 600
    r = _rand(17, n, k)
    r[::5, 0] = np.nan
    r[1::5, 1] = np.inf
    r[2::5, 2] = -np.inf
    r[3::5, 3] = 3e19                       # the square overflows to +INF
    q = _rand(18, 20, k)
    idx, dist = _check_whole(pkg, q, r, 64)
    assert (idx % 5 == 4).all()
    # fewer selectable refs than kn: the rest of the row is -1 / +INF
    idx, dist = _check_whole(pkg, q, r, 256)
    assert (idx[:, 120:] == -1).all() and np.isinf(dist[:, 120:]).all()
    assert (idx[:, :120] >= 0).all()


def test_fewer_refs_than_kn(pkg):
    q = _rand(19, 5, 3)
    r = _rand(20, 5, 3)
    idx, dist = _check_whole(pkg, q, r, 16)
    assert (idx[:, 5:] == -1).all() and np.isinf(dist[:, 5:]).all()
    assert (np.sort(idx[:, :5], axis=1) == np.arange(5)).all()


@pytest.mark.parametrize("k,m", [(1, 1), (1, 4), (3, 1), (3, 4)])
def test_many_splits_nearest_in_last_split(pkg, k, m):
    n, kn = 1 << 21, 20
    assert pkg.plan_topk(k, m, n, kn)["splits"] >= 64
    r = _rand(21 + k + m, n, k)
    q = _rand(22 + k + m, m, k) + np.float32(2.0)      # far from the cloud ...
    for i in range(m):
        for j in range(kn):                               # ... except kn planted refs in the last split
            r[n - 1 - j - kn * i] = q[i] + np.float32(1e-3 * (j + 1))
    idx, _ = _check_whole(pkg, q, r, kn)
    assert (idx >= n - kn * m).all()


def test_shards_give_identical_outputs(pkg):
    q = _rand(23, 70, 12)
    r = _rand(24, 20000, 12)
    idx1, dist1 = _check_whole(pkg, q, r, 50)
    for shards in (2, 3, 7):
        idx, dist = pkg.search_topk(q, r, 50, return_distances=True, shards=shards)
        _assert_same(idx, dist, idx1, dist1, f"shards={shards}")


def test_two_index_halves_merged_equal_one_index(pkg):
    dev = torch.device("cuda:0")
    n, k, kn = 9001, 24, 33
    rh = _rand(25, n, k)
    rh[4000:4600] = rh[5]                    # ties across the halves
    q = torch.from_numpy(_rand(26, 40, k)).to(dev)
    q[0] = torch.from_numpy(rh[5]).to(dev)
    r = torch.from_numpy(rh).to(dev)
    half = n // 2
    whole = pkg.Index(r)
    a = pkg.Index(r[:half].contiguous(), index_base=0)
    b = pkg.Index(r[half:].contiguous(), index_base=half)
    want = whole.search_topk_keys(q, kn)
    ka = a.search_topk_keys(q, kn)
    kb = b.search_topk_keys(q, kn)
    pkg.keys_topk_merge(ka, kb)
    torch.cuda.synchronize()
    assert torch.equal(ka, want)
    idx, dist = pkg.keys_topk_unpack(ka, return_distances=True)
    want_idx, want_dist = topk_oracle(q.cpu().numpy(), rh, kn)
    torch.cuda.synchronize()
    _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, "merged halves")
    for ix in (whole, a, b):
        ix.close()


def test_keys_topk_merge_pads_and_keeps_order(pkg):
    dev = torch.device("cuda:0")
    a = torch.tensor([[(1 << 32) | 3, (2 << 32) | 1, NONE, NONE]], dtype=torch.int64, device=dev)
    b = torch.tensor([[(1 << 32) | 0, NONE, NONE, NONE]], dtype=torch.int64, device=dev)
    pkg.keys_topk_merge(a, b)
    idx, dist = pkg.keys_topk_unpack(a, return_distances=True)
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == [[0, 3, 1, -1]]
    assert a[0, 3].item() == NONE and np.isinf(dist[0, 3].item())


def test_bf16_whole_call_and_index(pkg, orc):
    k, m, n, kn = 40, 33, 5000, 25
    qb = pkg.to_bf16_bits(_rand(27, m, k))
    rb = pkg.to_bf16_bits(_rand(28, n, k))
    q32 = (qb.astype(np.uint32) << 16).view(np.float32)
    r32 = (rb.astype(np.uint32) << 16).view(np.float32)
    want_idx, want_dist = topk_oracle(q32, r32, kn)
    for shards in (1, 3):
        idx, dist = pkg.search_topk_bf16(qb, rb, kn, return_distances=True, shards=shards)
        _assert_same(idx, dist, want_idx, want_dist, f"bf16 whole call shards={shards}")
    dev = torch.device("cuda:0")
    rt = torch.from_numpy(rb.view(np.int16)).to(dev).view(torch.bfloat16)
    qt = torch.from_numpy(qb.view(np.int16)).to(dev).view(torch.bfloat16)
    for path in ("auto", "mfma"):
        ix = pkg.Index(rt, path=path)
        idx, dist = ix.search_topk(qt, kn, return_distances=True)
        torch.cuda.synchronize()
        _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, f"bf16 index {path}")
        ix.close()


def test_dimension_major_refs(pkg):
    k, m, n, kn = 20, 17, 3000, 10
    q = _rand(29, m, k)
    r = _rand(30, n, k)
    want_idx, want_dist = topk_oracle(q, r, kn)
    rsoa = np.ascontiguousarray(r.T)
    for shards in (1, 2):
        idx, dist = pkg.search_topk(q, rsoa, kn, return_distances=True, refs_soa=True, shards=shards)
        _assert_same(idx, dist, want_idx, want_dist, f"soa shards={shards}")
    dev = torch.device("cuda:0")
    ix = pkg.Index(torch.from_numpy(rsoa).to(dev), soa=True, path="mfma")
    idx, dist = ix.search_topk(torch.from_numpy(q).to(dev), kn, return_distances=True)
    torch.cuda.synchronize()
    _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, "soa index")
    ix.close()


def test_caller_stream_and_device(pkg):
    dev = torch.device("cuda:0")
    k, m, n, kn = 64, 100, 30000, 16
    qh, rh = _rand(31, m, k), _rand(32, n, k)
    want_idx, want_dist = topk_oracle(qh, rh, kn)
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        q = torch.from_numpy(qh).to(dev)
        r = torch.from_numpy(rh).to(dev)
        ix = pkg.Index(r, stream=side)
        idx, dist = ix.search_topk(q, kn, return_distances=True, stream=side)
        idx_h, dist_h = idx.cpu(), dist.cpu()      # consumed on the side stream
    side.synchronize()
    assert torch.cuda.current_device() == 0
    _assert_same(idx_h.numpy(), dist_h.numpy(), want_idx, want_dist, "side stream")
    ix.close()
    pkg.search_topk(qh[:3], rh[:100], 4)
    assert torch.cuda.current_device() == 0


def test_alternating_searches_and_stats(pkg):
    dev = torch.device("cuda:0")
    k, m, n = 64, 300, 20000
    q = torch.from_numpy(_rand(33, m, k)).to(dev)
    r = torch.from_numpy(_rand(34, n, k)).to(dev)
    fresh = pkg.Index(r, path="mfma")
    want = fresh.search_keys(q).clone()
    fresh.close()
    ix = pkg.Index(r, path="mfma", profile=True)
    first = ix.search_keys(q).clone()
    assert ix.stats()["path"] == 2
    top = ix.search_topk_keys(q, 32)
    st = ix.stats()
    assert st["path"] == 1                   # NNS_PATH_EXACT
    assert st["exact_ms"] > 0 and st["total_ms"] > 0
    again = ix.search_keys(q)
    ix.search_topk_keys(q[:7], 200)          # another top-K shape between two 1-NN searches
    last = ix.search_keys(q)
    torch.cuda.synchronize()
    assert torch.equal(first, want) and torch.equal(again, want) and torch.equal(last, want)
    assert torch.equal(top[:, 0], want)
    ix.close()
