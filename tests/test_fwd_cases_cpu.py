"""CPU: the reference and the inputs of the per-element forward tests (tests/_fwd_cases.py).

  * the composition _fwd_cases.reference (numpy float32 prologue, then T times oracle.mdcn_c1 /
    prop_noffset, the preserve blend, the clamp) IS the float32 oracle's loop: bit for bit on the
    oracle's own normalised affinities, every iterate and pred, every input set;
  * the inputs are not degenerate: the ramp covers every distance on each axis and along the
    image's border, every _bwd_cases tap class occurs in every image, at least half of all taps
    sample inside the image;
  * the float32 oracle's affinity normalisation meets the recorded bar A32, and A32 stays under
    the operation-count ceiling.
"""
import numpy as np
import pytest

import _bwd_cases as bc
import _fwd_cases as fc

OFFSET_SETS = [n for n in fc.INPUTS if fc.INPUTS[n]["offset"]]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(fc.INPUTS))
def test_composition_is_the_oracle_loop(oracle, name):
    oracle.set_threads(16)
    s = fc.inputs(name)
    e = fc.oracle_propagate(oracle, name, s)
    p0, conf_b = fc.prologue(name, s)
    if fc.INPUTS[name]["conf"]:
        assert np.array_equal(_bits(conf_b), _bits(e["confidence"]))
    else:
        assert conf_b is None and e["confidence"] is None
    if fc.INPUTS[name]["offset"]:
        assert np.array_equal(_bits(e["offset"]), _bits(oracle.off_insert(s["off"])))
    inter, pred = fc.reference(oracle, name, s, e["aff"], e["offset"], e["confidence"])
    assert np.array_equal(_bits(inter), _bits(e["pred_inter"]))
    assert np.array_equal(_bits(pred), _bits(e["pred"]))
    assert np.isfinite(inter).all()


def test_ramp_shape():
    """Half-integer steps from -D to +D, rows for even taps and columns for odd ones, the other
    axis a common fractional tap; the cycle is odd."""
    off, d = fc.ramp_offsets(24, 40, 3, 3)
    assert fc.CYCLE % 2 == 1 and fc.CYCLE == 4 * fc.D + 1
    assert d.min() == -fc.D and d.max() == fc.D and np.array_equal(2 * d, np.round(2 * d))
    for k in range(8):
        ramp, other = (off[2 * k], off[2 * k + 1]) if k % 2 == 0 else (off[2 * k + 1], off[2 * k])
        assert np.array_equal(ramp, d[k])
        fr = other - np.floor(other)
        assert fr.min() >= 8 / 64 and fr.max() <= 56 / 64 and np.abs(other).max() < 3
    y, x, k = 5, 7, 3
    assert d[k, y, x] == ((x + 3 * y + 5 * k) % (4 * fc.D + 1)) / 2 - fc.D


@pytest.mark.parametrize("name", OFFSET_SETS)
def test_inputs_are_not_degenerate(name):
    c = fc.INPUTS[name]
    s = fc.inputs(name)
    B, H, W = c["B"], c["H"], c["W"]
    K = c["kh"] * c["kw"] - 1
    assert s["off"].shape == (B + 1, 2 * K, H, W) and s["aff"].shape == (B + 1, K, H, W)
    every = set(np.arange(fc.CYCLE) / 2.0 - fc.D)
    d = s["dist"]
    rows, cols = d[0::2], d[1::2]     # even taps ramp along the rows, odd taps along the columns
    # every distance on each axis ...
    assert set(rows.ravel()) == every and set(cols.ravel()) == every
    # ... and in the image's border frame (its first two and last two rows and columns), where the
    # image's own edge and a window's edge meet
    frame = np.zeros((H, W), bool)
    frame[:2] = frame[-2:] = frame[:, :2] = frame[:, -2:] = True
    assert set(rows[:, frame].ravel()) == every, sorted(every - set(rows[:, frame].ravel()))
    assert set(cols[:, frame].ravel()) == every, sorted(every - set(cols[:, frame].ravel()))
    # the ramp image's offsets are the ramp's, exactly
    assert np.array_equal(s["off"][B, 0::4], rows.astype(np.float32))
    assert np.array_equal(s["off"][B, 3::4], cols.astype(np.float32))
    assert np.all(s["cls"][B] == fc.RAMP)
    # every _bwd_cases class in every drawn image, by where the taps land
    h, w = fc.tap_coords(name, s)
    masks = fc.classify(h, w, H, W)
    for b in range(B):
        for i, cl in enumerate(bc.CLASSES):
            assert np.any(masks[b] >> i & 1), (b, cl)
        assert np.any(masks[b] == 0), (b, "common")
    # at least half of all taps sample inside the image
    inside = (h > -1) & (h < H) & (w > -1) & (w < W)
    print(f"{name}: {inside.mean():.3f} of the taps inside (ramp image {inside[B].mean():.3f})")
    assert inside.mean() >= 0.5
    assert np.abs(s["off"]).max() < 128 and np.array_equal(s["off"] * 64, np.round(s["off"] * 64))


@pytest.mark.parametrize("name", list(fc.INPUTS))
def test_affinity_bar(oracle, name):
    """The float32 oracle's normalisation against float64 on the same float32 planes: no worse than
    the tabled A32 of its kind, and A32 under the ceiling."""
    c = fc.INPUTS[name]
    s = fc.inputs(name)
    a64 = fc.aff_float64(oracle, name, s)
    a32 = oracle.affinity_normalization(s["aff"], c["kind"], fc.gamma_of(name))
    _, taps, ref = fc.aff_ratios(name, a32, a64)
    print(f"a32 {name} {c['kind']} taps {taps:.3e} ref {ref:.3e}")
    K = c["kh"] * c["kw"] - 1
    ceil, bar = fc.aff_ceiling(K), fc.A32[c["kind"]][K]
    assert taps <= bar[0] <= ceil, (taps, bar, ceil)
    assert ref <= bar[1] <= ceil, (ref, bar, ceil)
