"""CPU tests of the MFMA filter's configuration table (FILTER_CASES, no device): one shape per launch configuration
that nns_plan_filter can pick, where a configuration is the tile operator, the tau mode, shared or private lane
thresholds, the candidate-record form, K5's form (one row per query for 1 / 2-3 ref-range splits, one wave per query
from 4) and the stream length (long: more than 2048 32-ref tiles per split).  test_filter_configs_gpu.py runs every
case against the V0 oracle; the tests here keep the table exact (each case plans to its key), complete (a sweep of
the planner finds no key outside it) and cheap enough for the GPU suite's time budget."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_TILES = 2048                   # kShareThrMaxTiles and NNS_F_TILEREC_MAX (filter_mfma.hip)
ORACLE_BUDGET = 8e10                # checked queries x n x k per case (the CPU oracle does ~1e10 of these a second)
ORACLE_TOTAL = 3.7e12               # the same over the whole table
HOST_BYTES = 4 << 30                # peak host memory of one case

# dtype: "f32" (fp32 points and operands, tau mode 0), "bf16" (bf16 points, mode 1), "mixed" (fp32 points through
# bf16 operands, NNS_FILTER_BF16: mode 2), "f16" (fp16 points, filter_f16_kernel: tau mode 4) or "i8" (int8 points,
# filter_i8_kernel: 5, the form nns_index_filter_form reports; the planner reports bf16 = 1 for both, so their mode
# comes from the dtype).  per_ref: NNS_RECORDS_PER_REF (path "mfma_perref").  key: filter_key() of
# the plan, i.e. (kt, mode, share_thr, tile_rec, k5_form, long).  Long streams take the cheapest (m, n) of each K5
# form: splits = 1 needs >= 256 query groups, 2-3 and 4 splits need the ref count to grow with them.  k is below kt
# (ragged) in most cases, n is never a multiple of 32.
FilterCase = namedtuple("FilterCase", "dtype k m n per_ref key")
FILTER_CASES = [
    FilterCase("f32", 9, 131072, 65537, False, (16, 0, 0, 0, 'rows1', True)),
    FilterCase("f32", 9, 65536, 140001, False, (16, 0, 0, 0, 'rows2-3', True)),
    FilterCase("f32", 9, 32768, 300001, False, (16, 0, 0, 0, 'wave', True)),
    FilterCase("f32", 16, 250, 31, False, (16, 0, 1, 0, 'rows1', False)),
    FilterCase("f32", 13, 250, 777, False, (16, 0, 1, 0, 'rows2-3', False)),
    FilterCase("f32", 9, 250, 3001, True, (16, 0, 1, 0, 'wave', False)),
    FilterCase("f32", 16, 250, 3001, False, (16, 0, 1, 2, 'wave', False)),
    FilterCase("f32", 17, 131072, 65537, False, (32, 0, 0, 0, 'rows1', True)),
    FilterCase("f32", 17, 65536, 140001, False, (32, 0, 0, 0, 'rows2-3', True)),
    FilterCase("f32", 17, 32768, 300001, False, (32, 0, 0, 0, 'wave', True)),
    FilterCase("f32", 31, 250, 31, False, (32, 0, 1, 0, 'rows1', False)),
    FilterCase("f32", 17, 250, 300, False, (32, 0, 1, 0, 'rows2-3', False)),
    FilterCase("f32", 32, 250, 777, True, (32, 0, 1, 0, 'wave', False)),
    FilterCase("f32", 31, 250, 777, False, (32, 0, 1, 2, 'wave', False)),
    FilterCase("f32", 33, 131072, 65537, False, (64, 0, 0, 0, 'rows1', True)),
    FilterCase("f32", 33, 65536, 140001, False, (64, 0, 0, 0, 'rows2-3', True)),
    FilterCase("f32", 33, 32768, 300001, False, (64, 0, 0, 0, 'wave', True)),
    FilterCase("f32", 33, 250, 31, False, (64, 0, 1, 0, 'rows1', False)),
    FilterCase("f32", 64, 250, 140, False, (64, 0, 1, 0, 'rows2-3', False)),
    FilterCase("f32", 50, 250, 777, True, (64, 0, 1, 0, 'wave', False)),
    FilterCase("f32", 33, 250, 777, False, (64, 0, 1, 2, 'wave', False)),
    FilterCase("f32", 65, 131072, 65537, False, (128, 0, 0, 0, 'rows1', True)),
    FilterCase("f32", 65, 65536, 140001, False, (128, 0, 0, 0, 'rows2-3', True)),
    FilterCase("f32", 65, 32768, 300001, False, (128, 0, 0, 0, 'wave', True)),
    FilterCase("f32", 128, 250, 31, False, (128, 0, 1, 0, 'rows1', False)),
    FilterCase("f32", 127, 250, 100, False, (128, 0, 1, 0, 'rows2-3', False)),
    FilterCase("f32", 65, 250, 300, True, (128, 0, 1, 0, 'wave', False)),
    FilterCase("f32", 128, 250, 300, False, (128, 0, 1, 2, 'wave', False)),
    FilterCase("f32", 129, 65536, 65537, False, (256, 0, 0, 0, 'rows1', True)),
    FilterCase("f32", 129, 32768, 140001, False, (256, 0, 0, 0, 'rows2-3', True)),
    FilterCase("f32", 129, 16384, 300001, False, (256, 0, 0, 0, 'wave', True)),
    FilterCase("f32", 200, 250, 31, False, (256, 0, 1, 0, 'rows1', False)),
    FilterCase("f32", 129, 250, 63, False, (256, 0, 1, 0, 'rows2-3', False)),
    FilterCase("f32", 256, 250, 100, True, (256, 0, 1, 0, 'wave', False)),
    FilterCase("f32", 200, 250, 100, False, (256, 0, 1, 2, 'wave', False)),
    FilterCase("bf16", 100, 131072, 65537, False, (128, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 100, 65536, 140001, False, (128, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 100, 32768, 300001, False, (128, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 100, 250, 31, False, (128, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 128, 250, 140, False, (128, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 33, 250, 777, True, (128, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 100, 250, 777, False, (128, 1, 1, 1, 'wave', False)),
    FilterCase("bf16", 129, 131072, 65537, False, (256, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 129, 65536, 140001, False, (256, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 129, 32768, 300001, False, (256, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 256, 250, 31, False, (256, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 255, 250, 100, False, (256, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 129, 250, 300, True, (256, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 256, 250, 300, False, (256, 1, 1, 1, 'wave', False)),
    FilterCase("bf16", 257, 65536, 65537, False, (384, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 257, 32768, 140001, False, (384, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 257, 16384, 300001, False, (384, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 300, 250, 31, False, (384, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 257, 250, 140, False, (384, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 384, 250, 777, True, (384, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 300, 250, 777, False, (384, 1, 1, 2, 'wave', False)),
    FilterCase("bf16", 385, 65536, 65537, False, (512, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 385, 32768, 140001, False, (512, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 385, 16384, 300001, False, (512, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 385, 250, 31, False, (512, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 512, 250, 63, False, (512, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 511, 250, 100, True, (512, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 385, 250, 100, False, (512, 1, 1, 1, 'wave', False)),
    FilterCase("bf16", 513, 65536, 65537, False, (640, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 513, 32768, 140001, False, (640, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 513, 16384, 300001, False, (640, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 640, 250, 31, False, (640, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 600, 250, 140, False, (640, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 513, 250, 777, True, (640, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 640, 250, 777, False, (640, 1, 1, 2, 'wave', False)),
    FilterCase("bf16", 641, 65536, 65537, False, (768, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 641, 32768, 140001, False, (768, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 641, 16384, 300001, False, (768, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 700, 250, 31, False, (768, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 641, 250, 100, False, (768, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 768, 250, 300, True, (768, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 700, 250, 300, False, (768, 1, 1, 2, 'wave', False)),
    FilterCase("bf16", 769, 32768, 65537, False, (1024, 1, 0, 0, 'rows1', True)),
    FilterCase("bf16", 769, 16384, 140001, False, (1024, 1, 0, 0, 'rows2-3', True)),
    FilterCase("bf16", 769, 8192, 300001, False, (1024, 1, 0, 0, 'wave', True)),
    FilterCase("bf16", 769, 250, 31, False, (1024, 1, 1, 0, 'rows1', False)),
    FilterCase("bf16", 1024, 250, 63, False, (1024, 1, 1, 0, 'rows2-3', False)),
    FilterCase("bf16", 1000, 250, 100, True, (1024, 1, 1, 0, 'wave', False)),
    FilterCase("bf16", 769, 250, 100, False, (1024, 1, 1, 2, 'wave', False)),
    FilterCase("mixed", 100, 131072, 65537, False, (128, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 100, 65536, 140001, False, (128, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 100, 32768, 300001, False, (128, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 128, 250, 31, False, (128, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 33, 250, 140, False, (128, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 100, 250, 777, True, (128, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 128, 250, 777, False, (128, 2, 1, 1, 'wave', False)),
    FilterCase("mixed", 129, 131072, 65537, False, (256, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 129, 65536, 140001, False, (256, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 129, 32768, 300001, False, (256, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 255, 250, 31, False, (256, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 129, 250, 100, False, (256, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 256, 250, 300, True, (256, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 255, 250, 300, False, (256, 2, 1, 1, 'wave', False)),
    FilterCase("mixed", 257, 65536, 65537, False, (384, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 257, 32768, 140001, False, (384, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 257, 16384, 300001, False, (384, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 257, 250, 31, False, (384, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 384, 250, 140, False, (384, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 300, 250, 777, True, (384, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 257, 250, 777, False, (384, 2, 1, 2, 'wave', False)),
    FilterCase("mixed", 385, 65536, 65537, False, (512, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 385, 32768, 140001, False, (512, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 385, 16384, 300001, False, (512, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 512, 250, 31, False, (512, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 511, 250, 63, False, (512, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 385, 250, 100, True, (512, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 512, 250, 100, False, (512, 2, 1, 1, 'wave', False)),
    FilterCase("mixed", 513, 65536, 65537, False, (640, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 513, 32768, 140001, False, (640, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 513, 16384, 300001, False, (640, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 600, 250, 31, False, (640, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 513, 250, 140, False, (640, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 640, 250, 777, True, (640, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 600, 250, 777, False, (640, 2, 1, 2, 'wave', False)),
    FilterCase("mixed", 641, 65536, 65537, False, (768, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 641, 32768, 140001, False, (768, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 641, 16384, 300001, False, (768, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 641, 250, 31, False, (768, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 768, 250, 100, False, (768, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 700, 250, 300, True, (768, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 641, 250, 300, False, (768, 2, 1, 2, 'wave', False)),
    FilterCase("mixed", 769, 32768, 65537, False, (1024, 2, 1, 0, 'rows1', True)),
    FilterCase("mixed", 769, 16384, 140001, False, (1024, 2, 1, 0, 'rows2-3', True)),
    FilterCase("mixed", 769, 8192, 300001, False, (1024, 2, 1, 0, 'wave', True)),
    FilterCase("mixed", 1024, 250, 31, False, (1024, 2, 1, 0, 'rows1', False)),
    FilterCase("mixed", 1000, 250, 63, False, (1024, 2, 1, 0, 'rows2-3', False)),
    FilterCase("mixed", 769, 250, 100, True, (1024, 2, 1, 0, 'wave', False)),
    FilterCase("mixed", 1024, 250, 100, False, (1024, 2, 1, 2, 'wave', False)),
    FilterCase("f16", 100, 131072, 65537, False, (128, 4, 0, 0, 'rows1', True)),
    FilterCase("f16", 100, 65536, 140001, False, (128, 4, 0, 0, 'rows2-3', True)),
    FilterCase("f16", 100, 32768, 300001, False, (128, 4, 0, 0, 'wave', True)),
    FilterCase("f16", 100, 250, 31, False, (128, 4, 1, 0, 'rows1', False)),
    FilterCase("f16", 128, 250, 140, False, (128, 4, 1, 0, 'rows2-3', False)),
    FilterCase("f16", 33, 250, 777, True, (128, 4, 1, 0, 'wave', False)),
    FilterCase("f16", 100, 250, 777, False, (128, 4, 1, 1, 'wave', False)),
    FilterCase("f16", 129, 131072, 65537, False, (256, 4, 0, 0, 'rows1', True)),
    FilterCase("f16", 129, 65536, 140001, False, (256, 4, 0, 0, 'rows2-3', True)),
    FilterCase("f16", 129, 32768, 300001, False, (256, 4, 0, 0, 'wave', True)),
    FilterCase("f16", 256, 250, 31, False, (256, 4, 1, 0, 'rows1', False)),
    FilterCase("f16", 255, 250, 100, False, (256, 4, 1, 0, 'rows2-3', False)),
    FilterCase("f16", 129, 250, 300, True, (256, 4, 1, 0, 'wave', False)),
    FilterCase("f16", 256, 250, 300, False, (256, 4, 1, 1, 'wave', False)),
    FilterCase("i8", 100, 131072, 65537, False, (256, 5, 0, 0, 'rows1', True)),
    FilterCase("i8", 129, 65536, 140001, False, (256, 5, 0, 0, 'rows2-3', True)),
    FilterCase("i8", 200, 32768, 300001, False, (256, 5, 0, 0, 'wave', True)),
    FilterCase("i8", 256, 250, 31, False, (256, 5, 1, 0, 'rows1', False)),
    FilterCase("i8", 33, 250, 140, False, (256, 5, 1, 0, 'rows2-3', False)),
    FilterCase("i8", 129, 250, 777, True, (256, 5, 1, 0, 'wave', False)),
    FilterCase("i8", 100, 250, 777, False, (256, 5, 1, 1, 'wave', False)),
]


def filter_case_id(c):
    return f"{c.dtype}-k{c.k}-m{c.m}-n{c.n}" + ("-perref" if c.per_ref else "")


PLAN_DTYPE = {"bf16": 1, "f16": 2, "i8": 3}         # nns_plan_filter's bf16 argument
KEY_MODE = {"f16": 4, "i8": 5}                      # the key's mode field where the plan's bf16 / mixed do not tell


def plan_case(pkg, c):
    """The case's plan (plan_filter's fields) plus "dtype", the case's."""
    flags = (pkg.NNS_RECORDS_PER_REF if c.per_ref else 0) | (pkg.NNS_FILTER_BF16 if c.dtype == "mixed" else 0)
    p = pkg.plan_filter(c.k, c.m, c.n, bf16=PLAN_DTYPE.get(c.dtype, 0), flags=flags)
    p["dtype"] = c.dtype
    return p


def stream_tiles(p):
    """32-ref tiles in one split's ref stream (test_plan_cpu._check_plan's arithmetic: super-periods of the deep
    tiles, blocks of two slots at 1024-deep)."""
    kt, sps = p["kt"], p["slots_per_split"]
    if kt == 768:
        return sps * 2 // 3
    if kt == 640:
        return sps * 4 // 5
    if kt == 384:
        return sps * 4 // 3
    return sps * max(p["slot_pts"], 32) // 32 // (2 if kt == 1024 else 1)


def refs_per_split(p):
    """Refs of one ref-range split: slots_per_split / slots_per_block super-periods of pad_pts refs (filter_plan)."""
    # k-steps per block (mixed plans with bf16 = 1; an int8 fragment holds 64 dims of bytes, so OpI8 at kt 256 has
    # OpBF16K128's 8 steps).  p: plan_case's, or plan_filter's own for fp32 / bf16 points
    spb = p["kt"] // 32 if p.get("dtype") == "i8" else (p["kt"] // 16 if p["bf16"] else p["kt"] // 8)
    deep = 32 % spb != 0
    gcd = 32 if spb % 32 == 0 else (16 if spb % 16 == 0 else 8)
    slots_per_block = spb // gcd if deep else 1
    pad_pts = 32 * (32 // gcd) if deep else 32 * (32 // spb)
    return p["slots_per_split"] // slots_per_block * pad_pts


def filter_key(p):
    mode = KEY_MODE.get(p.get("dtype"), 2 if p["mixed"] else p["bf16"])
    assert p["bf16"] == 1 or p.get("dtype") not in KEY_MODE, p
    s = p["splits"]
    k5 = "rows1" if s == 1 else ("rows2-3" if s <= 3 else "wave")
    return (p["kt"], mode, p["share_thr"], p["tile_rec"], k5, stream_tiles(p) > LONG_TILES)


def checked_queries(c, planted):
    """(random sample, near-tie cap) of the queries the GPU test checks against the oracle over all refs: 512 random
    (256 above 512-D) and up to 2048 near-tie queries, fewer where that would overrun the case's oracle budget."""
    sample = min(c.m, 512 if c.k <= 512 else 256)
    near_cap = int(min(2048, max(0, ORACLE_BUDGET // (c.n * c.k) - sample - planted)))
    return sample, near_cap


def max_planted(c):
    """Most planted queries: exact copies and near-tie queries (none when m is tiny); < 1 % of m on the big cases."""
    return max(1, min(c.m // 4, 40))


def host_bytes(c):
    """Peak host memory of a case: fp32 queries and refs, the gathered refs of every answer, and the two key sets."""
    return 4 * (c.m * c.k * 2 + c.n * c.k) + 16 * c.m


def _libconst(pattern):
    src = open(os.path.join(ROOT, "nns-cuda_amd", "csrc", "filter_mfma.hip")).read()
    return int(re.search(pattern, src).group(1))


def test_long_stream_boundary_matches_the_library():
    assert _libconst(r"kShareThrMaxTiles\s*=\s*(\d+)") == LONG_TILES
    assert _libconst(r"#define NNS_F_TILEREC_MAX (\d+)") == LONG_TILES


@pytest.mark.parametrize("c", FILTER_CASES, ids=[filter_case_id(c) for c in FILTER_CASES])
def test_case_plans_to_its_key(pkg, c):
    p = plan_case(pkg, c)
    assert filter_key(p) == c.key, (c, p)
    assert refs_per_split(p) // 32 == stream_tiles(p)
    assert refs_per_split(p) * (p["splits"] - 1) < c.n <= refs_per_split(p) * p["splits"] or p["n_pad"] > c.n
    assert c.n % 32 != 0


def test_cases_are_distinct_and_ragged():
    keys = [c.key for c in FILTER_CASES]
    assert len(set(keys)) == len(keys) == 154
    kt = {c: c.key[0] for c in FILTER_CASES}
    assert sum(c.k != kt[c] for c in FILTER_CASES) * 2 >= len(FILTER_CASES)
    # every record / threshold form with private thresholds is reached at every depth that has it
    assert {(c.key[0], c.key[1]) for c in FILTER_CASES if c.key[2] == 0} == \
        {(kt_, 0) for kt_ in (16, 32, 64, 128, 256)} | {(kt_, 1) for kt_ in (128, 256, 384, 512, 640, 768, 1024)} | \
        {(128, 4), (256, 4), (256, 5)}


def _sweep_keys(pkg):
    ks_f = [1, 8, 16, 17, 32, 33, 64, 65, 128, 129, 256]
    ks_b = [8, 32, 128, 129, 256, 257, 384, 385, 512, 513, 640, 641, 768, 769, 1024]
    ms = [1, 63, 64, 512, 4096, 8192, 16384, 32768, 65536, 131072, 300000]
    ns = [1, 63, 1000, 65537, 140001, 300001, 1048576, 8388608]
    found = {}
    for dtype, ks in (("f32", ks_f), ("bf16", ks_b), ("mixed", ks_b), ("f16", [32, 33, 128, 129, 256]),
                      ("i8", [32, 128, 129, 256])):
        for k in ks:
            for m in ms:
                for n in ns:
                    for per_ref in (False, True):
                        c = FilterCase(dtype, k, m, n, per_ref, None)
                        found.setdefault(filter_key(plan_case(pkg, c)), c)
    return found


def test_cases_cover_every_reachable_configuration(pkg):
    """A brute-force sweep of the planner over a fixed grid finds exactly the table's keys: a planner change that adds a
    configuration fails here until a case for it is added."""
    found = _sweep_keys(pkg)
    table = {c.key for c in FILTER_CASES}
    assert not set(found) - table, f"configurations without a case: {sorted(set(found) - table)}"
    assert not table - set(found), f"cases the sweep does not reach: {sorted(table - set(found))}"


def test_cases_stay_inside_the_gpu_budget():
    total = 0.0
    for c in FILTER_CASES:
        sample, near_cap = checked_queries(c, max_planted(c))
        work = (sample + near_cap + max_planted(c)) * c.n * c.k
        assert work <= ORACLE_BUDGET * 1.0001, (c, work)
        assert host_bytes(c) <= HOST_BYTES, (c, host_bytes(c))
        assert c.m * c.n * c.k <= 2e13, c          # GPU work: a few hundred ms of MFMA at most
        total += work
    assert total <= ORACLE_TOTAL, total
    # the near-tie cap only shrinks below 2048 on the long streams of deep tiles, and never below 32
    assert min(checked_queries(c, max_planted(c))[1] for c in FILTER_CASES) >= 32
