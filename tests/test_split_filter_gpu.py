"""GPU tests of the two operand forms of fp32 points: the fp32-operand filter (NNS_FILTER_F32, K3's OpF32T) at every
fp32 configuration of FILTER_CASES — test_filter_configs_gpu.py runs the default split-bf16 form there — the split
chain of the MFMA self-test against fp64 and the mode-3 model, C3 at full size (keys of the two forms bit-equal, V0
parity on random and near-tie queries), and tight Gaussian clusters, where the margin decides how many queries fall
back to the exact scan."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_filter_configs_gpu as tfc  # noqa: E402
from test_filter_cases_cpu import FILTER_CASES, filter_case_id  # noqa: E402
from test_split_filter_cpu import _families, _split  # noqa: E402

pytestmark = pytest.mark.gpu

F32_CASES = [c for c in FILTER_CASES if c.dtype == "f32"]
U = 2.0 ** -24


@pytest.mark.timeout(600)
@pytest.mark.parametrize("c", F32_CASES, ids=[filter_case_id(c) for c in F32_CASES])
def test_fp32_operand_filter_configuration_vs_oracle(pkg, orc, c, monkeypatch):
    """test_filter_configs_gpu's check of one configuration, every index opened with NNS_FILTER_F32."""
    def open_f32(pkg_, c_, refs_dev, index_base=0):
        ix = pkg_.Index(refs_dev, index_base=index_base, path="mfma_perref" if c_.per_ref else "mfma", filter_f32=True)
        assert ix.stats()["filter_form"] == "fp32"
        return ix
    monkeypatch.setattr(tfc, "open_index", open_f32)
    tfc.test_filter_configuration_vs_oracle(pkg, orc, c)


@pytest.mark.parametrize("kt", [16, 32, 64, 128, 256])
def test_split_mfma_chain_error_model(pkg, kt):
    """The split chain on hardware (self-test mode 3: hi / lo parts, hi.hi + hi.lo + lo.hi per 16-dim step on
    v_mfma_f32_32x32x16_bf16) against fp64.  Its ACCUMULATION error — hardware against the exact sum of the three
    products, the part of the model that rests on an undocumented summation — must stay within 1/4 of the 2u-per-add
    bound on the actual magnitudes; its TOTAL error against the unsplit fp32 values within the e3 + e2 that
    nns_tau_consts reports for mode 3 (the truncation part of that bound is attained by midpoint data: the
    truncation itself is emulated exactly and checked in test_split_filter_cpu.py)."""
    rng = np.random.default_rng(31 + kt)
    na = 3 * kt + 3 * (kt // 16) + 2
    worst_acc = worst_tot = 0.0
    for name, x1, v1 in _families(rng, kt):
        if name.startswith("subnormal"):
            continue   # (denormal handling of the MFMA: the floor of tau; tests/test_underflow_gpu.py)
        # 32 queries / refs per family: the family's vectors, permuted and sign-flipped per row
        perm = [rng.permutation(kt) for _ in range(32)]
        x = np.stack([x1[p] for p in perm]).astype(np.float32)
        v = np.stack([v1[p] * np.float32(1 if i % 3 else -1) for i, p in enumerate(perm)]).astype(np.float32)
        c0 = ((v.astype(np.float64) / 2) ** 2).sum(1).astype(np.float32)   # |y'|^2, v = -2 y'
        out = pkg.selftest_mfma(v, x, c0, bf16=3).astype(np.float64)      # [ref i][query j]
        vh, vl = _split(v)
        xh, xl = _split(x)
        d = lambda t: t.astype(np.float64)   # noqa: E731
        prods = d(vh) @ d(xh).T + d(vh) @ d(xl).T + d(vl) @ d(xh).T
        absprods = np.abs(d(vh)) @ np.abs(d(xh)).T + np.abs(d(vh)) @ np.abs(d(xl)).T + np.abs(d(vl)) @ np.abs(d(xh)).T
        exact_split = d(c0)[:, None] + prods
        acc_err = np.abs(out - exact_split)
        acc_bound = 2 * na * U * (np.abs(d(c0))[:, None] + absprods)
        assert (acc_err <= 0.25 * acc_bound).all(), (kt, name, float((acc_err / acc_bound).max()))
        worst_acc = max(worst_acc, float((acc_err / acc_bound).max()))
        tot_err = np.abs(out - (d(c0)[:, None] + d(v) @ d(x).T))
        y2max = float(c0.max())
        for j in range(32):
            c0t, c1t, _ = pkg.tau_consts(kt, float((d(x[j]) ** 2).sum()), y2max, 3)
            bound = c0t / (2.0 + c1t) / 1.001
            worst_tot = max(worst_tot, float(tot_err[:, j].max() / bound))
            assert tot_err[:, j].max() <= bound, (kt, name, j)
    print(f"split chain kt {kt}: accumulation error / 2u-per-add bound {worst_acc:.4f}, total / mode-3 e3 {worst_tot:.4f}")


def _uniform(pkg, m, n, k, seed):
    q = torch.empty((m, k), dtype=torch.float32, device="cuda")
    r = torch.empty((n, k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, m * k)
    return q, r


@pytest.mark.timeout(900)
def test_c3_split_keys_equal_fp32_operands_and_v0(pkg, orc):
    """C3 at full size (65536 x 1048576 x 128, bench.py's data): the split and NNS_FILTER_F32 indices return the same
    keys bit for bit; no query needs the exact scan; V0 parity over all refs on 1024 random queries and every query
    K5 decided among several candidates (up to 1024 of them)."""
    m, n, k = 65536, 1048576, 128
    q, r = _uniform(pkg, m, n, k, 1000)
    ix = pkg.Index(r, path="auto")
    keys = ix.search_keys(q).clone()
    torch.cuda.synchronize()
    st = ix.stats()
    near = ix.near_ties()
    ix.close()
    assert st["filter_form"] == "split" and st["ambiguous"] == 0, st
    ix = pkg.Index(r, path="auto", filter_f32=True)
    keys32 = ix.search_keys(q)
    torch.cuda.synchronize()
    assert ix.stats()["filter_form"] == "fp32"
    ix.close()
    assert torch.equal(keys, keys32)
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    rng = np.random.default_rng(3)
    if near.size > 1024:
        near = rng.choice(near, 1024, replace=False)
    sel = np.unique(np.concatenate([rng.choice(m, 1024, replace=False), near]))
    qh, rh = q.cpu().numpy(), r.cpu().numpy()
    want_idx, want_dist = orc.v0_search(qh[sel], rh, threads=16)
    assert np.array_equal(idx_h[sel], want_idx)
    assert np.array_equal(dist_h[sel].view(np.uint32), want_dist.view(np.uint32))


def clustered(m, n, k, clusters, sigma, seed):
    """Tight Gaussian clusters: centres uniform in [0, 1)^k, refs and queries centre + sigma N(0, 1), refs in random
    cluster order.  Nearest-neighbour distances ~ 256 sigma^2 << |x'||y'| ~ k / 12."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.rand((clusters, k), generator=g, device="cuda")
    rc = torch.randint(0, clusters, (n,), generator=g, device="cuda")
    qc = torch.randint(0, clusters, (m,), generator=g, device="cuda")
    r = (centres[rc] + sigma * torch.randn((n, k), generator=g, device="cuda")).contiguous()
    q = (centres[qc] + sigma * torch.randn((m, k), generator=g, device="cuda")).contiguous()
    return q, r


@pytest.mark.timeout(900)
def test_clustered_data_stays_in_the_filter(pkg, orc):
    """65536 x 1048576 x 128 in 1024 tight clusters (sigma 0.03: nearest-neighbour distance ~0.2 against
    |x'||y'| ~ 11): the split form's margin (~2^-13 |x'||y'|) must leave at most 5 % of the queries to the exact scan — bf16-rounded operands (NNS_FILTER_BF16, ~2^-6) put whole
    clusters inside the margin — with keys bit-equal to the fp32-operand filter's and V0 parity on a sample."""
    m, n, k = 65536, 1048576, 128
    q, r = clustered(m, n, k, 1024, 0.03, 5)
    ix = pkg.Index(r, path="auto")
    keys = ix.search_keys(q).clone()
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    assert st["filter_form"] == "split"
    assert st["ambiguous"] <= m // 20, st
    ix = pkg.Index(r, path="auto", filter_f32=True)
    keys32 = ix.search_keys(q)
    torch.cuda.synchronize()
    ix.close()
    assert torch.equal(keys, keys32)
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    sel = np.random.default_rng(9).choice(m, 256, replace=False)
    want_idx, want_dist = orc.v0_search(q.cpu().numpy()[sel], r.cpu().numpy(), threads=16)
    assert np.array_equal(idx.cpu().numpy()[sel], want_idx)
    assert np.array_equal(dist.cpu().numpy()[sel].view(np.uint32), want_dist.view(np.uint32))
