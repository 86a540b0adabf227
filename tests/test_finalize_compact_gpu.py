"""GPU tests of K5's unit-wise kernel (finalize.hip, finalize_kernel: one wave per list unit — minimum, compaction of the
candidates into an LDS queue, dense evaluation with an LDS merge per query).  ring_pass_splits sends a shape there only
with many query groups of 512 (splits < 4: 128 groups -> 2 splits, 256 -> 1, and 3 only from 169 - 170 groups: below 86
groups three splits leave CUs idle and the plan takes four), so the shapes are large in m and small in n and k; every test
first requires the plan to say so.  The reference is the same data through the index's exact path (held against the oracle by the rest
of the suite) — keys equal means indices and distance bits equal — and the V0 oracle itself on 256 random queries."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"fp32": (torch.float32, False), "bf16": (torch.bfloat16, True), "fp16": (torch.float16, 2)}


def _queue_capacity():
    src = open(os.path.join(ROOT, "nns-cuda_amd", "csrc", "finalize.hip")).read()
    return int(re.search(r"constexpr int kK5Queue = (\d+);", src).group(1))


def _require_unit_kernel(pkg, k, m, n, points="fp32", splits=None):
    p = pkg.plan_filter(k, m, n, bf16=DTYPES[points][1])
    assert p["splits"] < 4 and p["tile_rec"] == 0, p
    if splits is not None:
        assert p["splits"] == splits, p
    return p


def _uniform(pkg, m, n, k, seed, points="fp32"):
    """Uniform [0, 1) queries and refs of the points' type on the device (fill_uniform: the oracle's RNG)."""
    q = torch.empty((m, k), dtype=torch.float32, device="cuda")
    r = torch.empty((n, k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, m * k)
    dt = DTYPES[points][0]
    return q.to(dt).contiguous(), r.to(dt).contiguous()


def _search(pkg, q, r, path, index_base=0):
    """(keys, stats, near ties) of one search."""
    ix = pkg.Index(r, path=path, index_base=index_base)
    keys = ix.search_keys(q).clone()
    torch.cuda.synchronize()
    st = ix.stats()
    ties = ix.near_ties() if path == "mfma" else None
    ix.close()
    return keys, st, ties


def _check_oracle_sample(pkg, orc, q, r, keys, seed, index_base=0):
    """256 random queries against the V0 oracle: indices and distance bits."""
    sel = np.sort(np.random.default_rng(seed).choice(q.shape[0], 256, replace=False))
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    idx, dist = idx.cpu().numpy()[sel], dist.cpu().numpy()[sel]
    qs = q[torch.from_numpy(sel).cuda()].float().cpu().numpy()
    want_idx, want_dist = orc.v0_search(qs, r.float().cpu().numpy(), threads=16)
    assert np.array_equal(idx.astype(np.int64), want_idx.astype(np.int64) + index_base), sel[np.nonzero(idx != want_idx + index_base)[0][:5]]
    assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))


# ---- parity over the instantiations ---------------------------------------------------------------------------------
#        points  k    m           n     splits  index_base
CASES = [("fp32", 128, 65536 - 37, 8192, 2, 0),           # lazy-16 lists, lpq 2, a ragged last unit
         ("fp32", 16, 87040, 4096, 3, 1000003),           # three splits (of 3, 3 and 2 ring slots); a non-zero index base
         ("fp32", 32, 131072, 4096, 1, 0),                # one split
         ("bf16", 256, 65536, 8192, 2, 0),                # lpq 4: 16-query units
         ("fp16", 128, 65536, 8192, 2, 0)]


@pytest.mark.parametrize("points,k,m,n,splits,base", CASES, ids=[f"{c[0]}_k{c[1]}_m{c[2]}_s{c[4]}" for c in CASES])
def test_unit_kernel_equals_the_exact_path(pkg, orc, points, k, m, n, splits, base):
    p = _require_unit_kernel(pkg, k, m, n, points, splits)
    if points == "bf16":
        assert p["lpq"] == 4, p
    q, r = _uniform(pkg, m, n, k, 2100 + k + splits, points)
    keys, st, _ = _search(pkg, q, r, "mfma", base)
    assert st["path"] == 2 and st["splits"] == splits and st["nonfinite"] == 0, st
    assert st["ambiguous"] <= m // 100, st                # answered by K5, not by the exact scan behind it
    want, _, _ = _search(pkg, q, r, "exact", base)
    assert torch.equal(keys, want), torch.nonzero(keys != want)[:5].flatten().tolist()
    _check_oracle_sample(pkg, orc, q, r, keys, 7 + k, base)


# ---- two copies of every ref ----------------------------------------------------------------------------------------
def test_two_copies_lower_index_wins_and_every_query_is_a_near_tie(pkg, orc):
    """Ref j + n/2 equals ref j: both copies are within the threshold of every query (in different splits), so every
    query's slot merges two candidates — ncand > 1 has to survive the LDS merge — and the lower index is V0's answer."""
    m, n, k = 65536, 8192, 128
    _require_unit_kernel(pkg, k, m, n, splits=2)
    q, r = _uniform(pkg, m, n, k, 2200)
    r[n // 2:] = r[:n // 2]
    keys, st, ties = _search(pkg, q, r, "mfma")
    assert st["ambiguous"] == 0, st
    idx = pkg.keys_unpack(keys).cpu().numpy()
    assert (idx < n // 2).all(), np.nonzero(idx >= n // 2)[0][:5]
    assert np.array_equal(ties, np.arange(m)), (ties.size, m)
    assert st["multi_candidate"] == m, st
    want, _, _ = _search(pkg, q, r, "exact")
    assert torch.equal(keys, want)
    _check_oracle_sample(pkg, orc, q, r, keys, 22)


# ---- many candidates per unit: the drain loop -----------------------------------------------------------------------
def test_eight_copies_drain_the_queue_more_than_twice_per_unit(pkg, orc):
    """1024 distinct points, each eight times (copy c at index p + 1024 c): a query's eight nearest refs tie, so a
    32-query unit holds 256 candidates plus the near ties of its queries' second-nearest points — more than twice the
    queue's capacity: the queue is drained inside the walk, again and again.  The candidates of a unit are counted on the
    host first, in float64 with the library's own threshold constants (tau_consts, mode 3): refs whose score
    |y'|^2 - 2 x'.y' is within a + tau(a) / 2 of the query's minimum a (half the margin: the filter's own scores may differ
    from float64 by a quarter of tau each at the very most, and measure far less).  No list overflows (11 - 21 of 64 entries in the CPU
    model of the record process), so the exact scan behind K5 cannot stand in for the queue."""
    m, n, k, distinct = 65536, 8192, 128, 1024
    cap = _queue_capacity()
    assert cap <= 128, "with a queue above 128 entries this test needs sixteen copies"
    _require_unit_kernel(pkg, k, m, n, splits=2)
    q, r = _uniform(pkg, m, n, k, 2300)
    r[:] = r[:distinct].repeat(n // distinct, 1)
    # host model of the first 64 units' candidates
    nq = 64 * 32
    rd = r[:distinct].double().cpu().numpy()
    qd = q[:nq].double().cpu().numpy()
    c = rd.mean(0)
    y, x = rd - c, qd - c
    y2, x2 = (y ** 2).sum(1), (x ** 2).sum(1)
    s = y2[None, :] - 2.0 * x @ y.T
    a = s.min(1)
    hits = np.zeros(nq, np.int64)
    for i in range(nq):
        c0, c1, x2c = pkg.tau_consts(k, float(x2[i]), float(y2.max()), 3)
        hits[i] = 8 * int((s[i] <= a[i] + 0.5 * (c0 + c1 * max(a[i] + x2c, 0.0))).sum())
    per_unit = hits.reshape(64, 32).sum(1)
    print(f"host model: {hits.mean():.2f} candidates per query, per 32-query unit {per_unit.min()} .. {per_unit.max()}, queue {cap}")
    assert per_unit.max() > 2 * cap, (per_unit.max(), cap)
    keys, st, ties = _search(pkg, q, r, "mfma")
    assert st["ambiguous"] <= m // 100, st
    assert ties.size == m - st["ambiguous"], (ties.size, st)   # every query K5 answered merged eight candidates or more
    idx = pkg.keys_unpack(keys).cpu().numpy()
    assert (idx < distinct).all()                         # the first of the eight copies
    want, _, _ = _search(pkg, q, r, "exact")
    assert torch.equal(keys, want), torch.nonzero(keys != want)[:5].flatten().tolist()
    _check_oracle_sample(pkg, orc, q, r, keys, 23)


# ---- fallbacks stay fallbacks ---------------------------------------------------------------------------------------
def test_a_nan_ref_sends_every_query_to_the_exact_scan(pkg, orc):
    """The NaN arrives with a refresh, which leaves the decision to the device: the search runs the filter and K5's check of
    K2's max-|value| word makes every query a fallback (an index created over such refs never runs the filter)."""
    m, n, k = 65536, 4096, 16
    _require_unit_kernel(pkg, k, m, n, splits=2)
    q, r = _uniform(pkg, m, n, k, 2400)
    ix = pkg.Index(r, path="mfma")
    r[1234, 5] = float("nan")
    ix.refresh()
    keys = ix.search_keys(q).clone()
    torch.cuda.synchronize()
    st, ties = ix.stats(), ix.near_ties()
    ix.close()
    assert st["path"] == 2 and st["ambiguous"] == m and st["nonfinite"] == 1, st
    assert ties.size == 0
    want, _, _ = _search(pkg, q, r, "exact")
    assert torch.equal(keys, want)
    assert (pkg.keys_unpack(keys).cpu().numpy() != 1234).all()   # V0 never selects a NaN distance
    _check_oracle_sample(pkg, orc, q, r, keys, 24)


def test_identical_refs_overflow_the_lists_and_answer_index_zero(pkg, orc):
    m, n, k = 65536, 4096, 16
    _require_unit_kernel(pkg, k, m, n, splits=2)
    q, r = _uniform(pkg, m, n, k, 2500)
    r[:] = r[0]
    keys, st, ties = _search(pkg, q, r, "mfma")
    assert st["path"] == 2 and st["ambiguous"] == m, st   # every list overflowed
    assert ties.size == 0
    assert (pkg.keys_unpack(keys).cpu().numpy() == 0).all()
    want, _, _ = _search(pkg, q, r, "exact")
    assert torch.equal(keys, want)
    _check_oracle_sample(pkg, orc, q, r, keys, 25)
