"""CPU: the case table of tests/_big_cases.py is what it claims (every row's last items start beyond
its tier, in bytes and in elements; no 2^31 / 2^32 displacement is invisible to the periodic
batch; the memory stays within the cap) and the slab comparator flags a wrapped read."""
import numpy as np
import pytest

import _big_cases as big
import _bwd_cases as bc

NAMES = [r["name"] for r in big.ROWS]


@pytest.mark.parametrize("name", NAMES)
def test_row_crosses_its_tier(name):
    r = big.ROW[name]
    lim, unit = big.TIERS[r["tier"]]
    n = big.n_items(r)
    for item in (n - 2, n - 1):  # two whole items start beyond the boundary ...
        b, e = big.start_offsets(r, item)
        assert b == e * r["es"]
        assert (b if unit == "bytes" else e) > lim, (item, b, e)
    # ... and the batch is the smallest with that property
    fewer = (r["B"] - 1) * r["items_per_batch"]
    b, e = big.start_offsets(r, fewer - 2)
    assert (b if unit == "bytes" else e) <= lim
    assert r["tier"] in big.crossed_tiers(r)
    # every row crosses S2 and therefore S1, except the 3x3 resident row (the plan's 64 groups x 256
    # parts hold less than 2^32 bytes of packed input: _big_cases.ROWS)
    want = {"S1"} if name == "prop_res_s1" else {"S1", "S2"}
    assert want <= set(big.crossed_tiers(r)), big.crossed_tiers(r)
    if r["tier"] == "S3":
        assert big.start_offsets(r, n - 2)[1] > 1 << 31


def test_cheap_rows_cross_s3():
    s3 = {n for n in NAMES if "S3" in big.crossed_tiers(big.ROW[n])}
    assert {"prop_f32_s3", "prop_f16_s3", "affnorm_f32_s3", "affnorm_f16_s3", "heads_fp32_s3"} <= s3


@pytest.mark.parametrize("name", NAMES)
def test_row_period_and_memory(name):
    r = big.ROW[name]
    assert r["k"] % 2 == 1 and r["k"] >= 3
    assert big.row_alias_free(r)
    assert r["W"] % 4 == 0 or not r.get("vector", True)  # the vector builds, where an entry has any
    assert big.peak_bytes(r) <= big.MEM_CAP, big.peak_bytes(r) / big.GIB
    if r["items_per_batch"] > 1:
        return
    s = big.sparse_items(r)
    assert s[0] == 0 and s[-1] == r["B"] - 1 and len(set(s)) == len(s) <= 2 + len(big.crossed_tiers(r))
    for t in big.crossed_tiers(r):              # the first item beyond each boundary, and the one before is not
        lim = big.tier_units(t, r["es"])
        first = [i for i in s if big.start_offsets(r, i)[0] > lim][0]
        assert big.start_offsets(r, first - 1)[0] <= lim < big.start_offsets(r, first)[0]


def test_alias_check_sees_an_invisible_wrap():
    """A displacement of a whole number of periods would be invisible; the check says so."""
    assert not big.alias_free(1 << 20, 4, 1, 1 << 12)            # k = 1: every item the same
    item = 1 << 10                                               # 2^31 bytes = 2^19 items of 4 KiB: a multiple of k = 2^3
    assert not big.alias_free(item, 4, 8, 1 << 21)
    assert big.alias_free(item, 4, 5, 1 << 21)                   # 2^19, 2^20, 2^21 and 2^22 items: never a multiple of 5
    assert big.alias_free(3 * item, 4, 3, 1 << 21)               # not a whole number of items


def test_compact_batch_is_the_bwd_case():
    c = bc.CASES["big_compact"]
    for n in ("prop_f32_s2", "prop_f32_s3", "prop_bwd_s2"):
        r = big.ROW[n]
        assert (c["H"], c["W"], c["kh"], c["kw"], c["T"]) == (r["H"], r["W"], r["kh"], r["kw"], r["T"])
        assert r["k"] == c["B"] + 1
    assert len(big.sparse_items(big.ROW["prop_bwd_s2"])) == c["B"]  # one image per non-zero item of the sparse batch
    assert set(bc.R32["big_compact"]) == set(bc.TENSORS)


def _wrapped(k, item, n, threshold, rng):
    """(compact, correct output, output of a kernel whose element offsets wrap at `threshold`)."""
    compact = rng.integers(1, 1 << 20, (k, item)).astype(np.float32)
    compact[k - 1] = 0
    good = big.fill_periodic(np.empty((n, item), np.float32), compact)
    flat = good.reshape(-1)
    idx = np.arange(flat.size)
    wrapped = flat[np.where(idx >= threshold, idx % threshold, idx)].reshape(n, item)
    return compact, good, wrapped


@pytest.mark.parametrize("k,item,n,threshold", [
    (3, 12, 40, 96), (3, 12, 41, 128), (5, 6, 57, 64), (5, 24, 33, 256), (3, 48, 11, 256), (5, 12, 23, 128), (5, 8, 40, 64),
])
@pytest.mark.parametrize("slab", [1, 200, 1 << 20])
def test_comparator_flags_a_wrap(k, item, n, threshold, slab):
    rng = np.random.default_rng(k * 1000 + item)
    compact, good, wrapped = _wrapped(k, item, n, threshold, rng)
    assert (threshold % item != 0) or (threshold // item) % k != 0  # the toy displacement is no whole number of periods
    assert big.first_mismatch(good, compact, slab) is None
    assert big.first_mismatch(wrapped, compact, slab) == threshold // item  # the first item that holds a wrapped element


def test_comparator_is_bitwise():
    compact = np.zeros((3, 4), np.float32)
    out = big.fill_periodic(np.empty((7, 4), np.float32), compact)
    assert big.first_mismatch(out, compact) is None
    out[5, 2] = -0.0                            # equal as a float, another bit pattern
    assert big.first_mismatch(out, compact) == 5
    out[5, 2] = 0.0
    out[6, 0] = np.nan                          # in the tail behind the last whole period
    assert big.first_mismatch(out, compact) == 6
    nan = np.full((3, 4), np.nan, np.float32)
    assert big.first_mismatch(big.fill_periodic(np.empty((7, 4), np.float32), nan), nan) is None


def test_sparse_helpers():
    t = np.zeros((9, 2, 3), np.float32)
    dense = np.arange(1, 19, dtype=np.float32).reshape(3, 2, 3)
    big.scatter_sparse(t, [0, 4, 8], dense)
    assert not big.nonzero_outside(t, [0, 4, 8]) and np.array_equal(t[4], dense[1])
    t[5, 1, 1] = -0.0
    assert not big.nonzero_outside(t, [0, 4, 8])
    t[5, 1, 1] = 1e-30
    assert big.nonzero_outside(t, [0, 4, 8])
    t[5, 1, 1] = np.nan
    assert big.nonzero_outside(t, [0, 4, 8])
