"""GPU tests of the lazy schedule of the split-bf16 filter (OpLazySplitT; the default of fp32 points at KT = 128 on long
streams — test_filter_configs_gpu.py and test_split_filter_gpu.py therefore run it unedited): the self-test's lazy chain
against fp64 and its hi-hi partial against B; every fp32 configuration of FILTER_CASES on the EAGER schedule
(NNS_FILTER_SPLIT_EAGER); C3 at full size with lazy, eager and fp32-operand keys bit-equal; and an input that needs B."""
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
LAZY_KTS = (128,)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("c", F32_CASES, ids=[filter_case_id(c) for c in F32_CASES])
def test_eager_split_filter_configuration_vs_oracle(pkg, orc, c, monkeypatch):
    """test_filter_configs_gpu's check of one configuration, every index opened with NNS_FILTER_SPLIT_EAGER."""
    def open_eager(pkg_, c_, refs_dev, index_base=0):
        ix = pkg_.Index(refs_dev, index_base=index_base, path="mfma_perref" if c_.per_ref else "mfma",
                        filter_split_eager=True)
        assert ix.stats()["filter_form"] == "split"
        return ix
    monkeypatch.setattr(tfc, "open_index", open_eager)
    tfc.test_filter_configuration_vs_oracle(pkg, orc, c)


@pytest.mark.parametrize("kt", [16, 32, 64, 128, 256])
def test_lazy_mfma_chain_error_model_and_bound(pkg, kt):
    """The lazy order on hardware (kt / 16 hi.hi MFMAs, then hi.lo and lo.hi of every step on the same accumulator):
    accumulation error within 1/4 of the 2u-per-add bound of the mode-3 model (order-free), total error within mode 3's
    e3 + e2; and the hi.hi partial is never more than B above the finished score."""
    rng = np.random.default_rng(57 + kt)
    na = 3 * kt + 3 * (kt // 16) + 2
    worst_acc = worst_b = 0.0
    for name, x1, v1 in _families(rng, kt):
        if name.startswith("subnormal"):
            continue   # (denormal handling of the MFMA: the floor of tau and B; tests/test_underflow_gpu.py)
        perm = [rng.permutation(kt) for _ in range(32)]
        x = np.stack([x1[p] for p in perm]).astype(np.float32)
        v = np.stack([v1[p] * np.float32(1 if i % 3 else -1) for i, p in enumerate(perm)]).astype(np.float32)
        c0 = ((v.astype(np.float64) / 2) ** 2).sum(1).astype(np.float32)   # |y'|^2, v = -2 y'
        out, out_hh = pkg.selftest_mfma_lazy(v, x, c0)                     # [ref i][query j]
        out, out_hh = out.astype(np.float64), out_hh.astype(np.float64)
        vh, vl = _split(v)
        xh, xl = _split(x)
        d = lambda t: t.astype(np.float64)   # noqa: E731
        prods = d(vh) @ d(xh).T + d(vh) @ d(xl).T + d(vl) @ d(xh).T
        absprods = np.abs(d(vh)) @ np.abs(d(xh)).T + np.abs(d(vh)) @ np.abs(d(xl)).T + np.abs(d(vl)) @ np.abs(d(xh)).T
        acc_err = np.abs(out - (d(c0)[:, None] + prods))
        acc_bound = 2 * na * U * (np.abs(d(c0))[:, None] + absprods)
        assert (acc_err <= 0.25 * acc_bound).all(), (kt, name, float((acc_err / acc_bound).max()))
        worst_acc = max(worst_acc, float((acc_err / acc_bound).max()))
        hh_err = np.abs(out_hh - (d(c0)[:, None] + d(vh) @ d(xh).T))
        assert (hh_err <= 0.25 * acc_bound).all(), (kt, name)
        tot_err = np.abs(out - (d(c0)[:, None] + d(v) @ d(x).T))
        y2max = float(c0.max())
        for j in range(32):
            x2 = float((d(x[j]) ** 2).sum())
            c0t, c1t, _ = pkg.tau_consts(kt, x2, y2max, 3)
            assert tot_err[:, j].max() <= c0t / (2.0 + c1t) / 1.001, (kt, name, j)
            B = pkg.split_lazy_bound(kt, x2, y2max)
            gap = float((out_hh[:, j] - out[:, j]).max())
            assert gap <= B, (kt, name, j, gap, B)
            worst_b = max(worst_b, gap / B)
    print(f"lazy chain kt {kt}: accumulation error / 2u-per-add bound {worst_acc:.4f}, (s_hh - s_3) / B {worst_b:.4f}")


def _uniform(pkg, m, n, k, seed):
    q = torch.empty((m, k), dtype=torch.float32, device="cuda")
    r = torch.empty((n, k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, m * k)
    return q, r


@pytest.mark.timeout(900)
def test_c3_lazy_eager_and_fp32_operand_keys_equal(pkg):
    """C3 at full size (65536 x 1048576 x 128, bench.py's data): the lazy (default), eager and fp32-operand indices
    return the same keys bit for bit, and no query of any of them needs the exact scan."""
    m, n, k = 65536, 1048576, 128
    assert pkg.plan_filter(k, m, n, schedule=True)["lazy"] == 1
    q, r = _uniform(pkg, m, n, k, 1000)
    got = {}
    for name, kw in (("lazy", {}), ("eager", {"filter_split_eager": True}), ("fp32", {"filter_f32": True})):
        ix = pkg.Index(r, path="auto", **kw)
        got[name] = ix.search_keys(q).clone()
        torch.cuda.synchronize()
        st = ix.stats()
        ix.close()
        assert st["filter_form"] == ("fp32" if name == "fp32" else "split") and st["ambiguous"] == 0, (name, st)
    assert torch.equal(got["lazy"], got["eager"])
    assert torch.equal(got["lazy"], got["fp32"])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kt", LAZY_KTS)
def test_true_nearest_ref_needs_the_bound(pkg, orc, kt):
    """A group of queries whose true nearest ref T has every cross term of x'.y' positive and at its maximum (hi-midpoint
    values 1 + 2^-8, equal signs: the finished score lies ~2^-6 |x'||y'| BELOW the hi-hi score) and arrives in the lane's
    stream AFTER a ref E that is farther by less than that.  In numpy first: T's hi-hi score is above the threshold E
    leaves, so a kernel testing against thr alone (B = 0) would retire T's tile unseen.  Then V0's index and distance
    bits are required from the GPU.  Long stream (C3's shape: two ref ranges of 16384 tiles, per-score records).
    The refs come in +- pairs of multiples of 2^-16: their fp64 sums are exact, the mean K2 subtracts is exactly 0 and
    the centred operands are the values themselves."""
    m, n, k = 65536, 1048576, kt
    p = pkg.plan_filter(k, m, n, schedule=True)
    assert p["lazy"] == 1 and p["kt"] == kt and p["tile_rec"] == 0 and p["share_thr"] == 0, p
    rng = np.random.default_rng(99)
    half = (rng.integers(-2 ** 15, 2 ** 15, (n // 2, k)) * 2.0 ** -16).astype(np.float32)
    mid = np.float32(1.0 + 2.0 ** -8)
    qg = np.full(k, mid, np.float32)
    T = qg.copy()
    E = (qg + np.float32(2.0 ** -4) * np.where(np.arange(k) % 2 == 0, 1, -1)).astype(np.float32)
    jE, jT = 64 * 10, 64 * 1000     # row 0 of their 32-ref blocks: the same lane half; both in the first ref range
    assert jT < p["slots_per_split"] * p["slot_pts"]
    half[jE], half[jT] = E, T
    r = np.concatenate([half, -half]).astype(np.float32)
    q = rng.random((m, k), dtype=np.float32) - np.float32(0.5)
    grp = np.arange(4096, 4096 + 64)
    q[grp] = qg
    # --- numpy: what the lane of a group query holds after E, and T's two scores
    d = lambda t: t.astype(np.float64)   # noqa: E731
    X2 = float((d(qg) ** 2).sum())
    ymax2 = float((d(r) ** 2).sum(1).max())
    qh, ql = _split(qg)

    def scores(y):
        vh, vl = _split((np.float32(-2) * y).astype(np.float32))
        s_hh = float((d(y) ** 2).sum() + d(qh) @ d(vh))
        return s_hh, s_hh + float(d(qh) @ d(vl) + d(ql) @ d(vh))
    _, s3_E = scores(E)
    shh_T, s3_T = scores(T)
    c0, c1, x2 = pkg.tau_consts(kt, X2, ymax2, 3)
    acc_slack = 2 * (3 * kt + 3 * (kt // 16) + 2) * U * (ymax2 + 4 * np.sqrt(X2 * ymax2))   # hardware summation
    thr_E = s3_E + acc_slack + 1.002 * (c0 + c1 * max(s3_E + acc_slack + x2, 0.0)) * (1 + 4 * U)
    B = pkg.split_lazy_bound(kt, X2, ymax2)
    assert s3_T + acc_slack < s3_E - acc_slack                # T is the nearer one also to the filter
    assert shh_T - acc_slack > thr_E, (shh_T, thr_E)          # ... but its hi-hi score is above the threshold E leaves
    assert shh_T - s3_T <= B                                  # and B is what brings its tile back
    want_idx, want_dist = orc.v0_search(q[grp], r, threads=16)
    assert (want_idx == jT).all() and (want_dist == 0).all()
    # --- the GPU
    ix = pkg.Index(torch.from_numpy(r).cuda(), path="mfma")
    keys = ix.search_keys(torch.from_numpy(q).cuda())
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    assert st["filter_form"] == "split" and st["k_tile"] == kt, st
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    assert np.array_equal(idx.cpu().numpy()[grp], want_idx)
    assert np.array_equal(dist.cpu().numpy()[grp].view(np.uint32), want_dist.view(np.uint32))
