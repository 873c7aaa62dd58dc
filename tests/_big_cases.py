"""The case table and the two input constructions of tests/test_gpu_big_offsets.py, in pure Python
(numpy only; the device helpers take torch tensors but import nothing), checked by
tests/test_big_cases_cpu.py.

Tiers.  A row makes ONE operand of an entry large enough that its last items start beyond

    S1  2^31 bytes        S2  2^32 bytes        S3  2^31 elements

from the tensor's base: where a 32-bit signed byte offset, a 32-bit unsigned byte offset and a
32-bit signed element index wrap.  B is the smallest batch for which at least two whole items
start beyond the tier (batch_for).  Images are the smallest the entry's vector builds take (W % 4
== 0, a few tiles), so a row costs memory traffic and no arithmetic to speak of.

Periodic batch (entries whose result for an image depends on that image alone).  Item b of every
operand is item b mod k of a compact batch of k items built on the host; k is odd and >= 3 and the
last compact item is all zeros.  The entry's output on the whole batch must then be its output on
the compact batch, tiled: first_mismatch() compares it bit for bit in slabs on the device (no host
copy, no second full-size tensor).  A kernel that truncates an item's offset by D reads or writes
D bytes lower; alias_free() shows that for D = 2^31 or 2^32 bytes or elements this never lands on
an item of the same residue mod k, for any operand of the row: every item size here has the
factor 3 (H * W = 3 * 2^n), so D is never a whole number of items and a wrapped access straddles
two items, of which at most one is the zero item.  (The GRU-mode rows have power-of-two item sizes
and k = 3: there D is a whole number 2^n of items, never a multiple of 3, and lands on another,
different compact item.)

Sparse batch (results summed over the batch).  Every item is zero except item 0, the first item
starting beyond each tier boundary the row crosses and item B - 1 (sparse_items); they hold the
compact batch's non-zero images in that order.  Zero items add exactly nothing to a sum, so the
result meets the entry's existing per-element bar against float64 on the non-zero items alone.

The compact propagation batch is _bwd_cases.CASES["big_compact"] (4 images of 24 x 32, K = 8, TGASS,
confidence, preserve, T = 3: tied to float64 per element by tests/test_gpu_backward_elem.py and
tests/test_oracle_backward.py like every other case) plus the zero item: k = 5.
"""
import numpy as np

TIERS = {"S1": (1 << 31, "bytes"), "S2": (1 << 32, "bytes"), "S3": (1 << 31, "elements")}
# what a truncated offset is off by: (amount, unit)
DISPLACEMENTS = ((1 << 31, "bytes"), (1 << 32, "bytes"), (1 << 31, "elements"), (1 << 32, "elements"))
ES = {"f32": 4, "f16": 2}
GIB = 1 << 30
MEM_CAP = 48 * GIB      # a sixth of the card
SLAB_BYTES = 256 << 20  # the comparator's temporaries stay below this


def tier_units(tier, es):
    """The tier's boundary in bytes."""
    n, unit = TIERS[tier]
    return n if unit == "bytes" else n * es


def batch_for(item_elems, es, tier):
    """The smallest item count for which at least two whole items start beyond the tier: items
    n - 2 and n - 1 have start offsets > the boundary."""
    return tier_units(tier, es) // (item_elems * es) + 3


def _row(name, entry, tensor, dtype, tier, k, operands, items_per_batch=1, **geom):
    es = ES[dtype]
    n = batch_for(operands[tensor], es, tier)
    B = -(-n // items_per_batch)
    return dict(name=name, entry=entry, tensor=tensor, dtype=dtype, es=es, tier=tier, k=k, operands=operands,
                items_per_batch=items_per_batch, B=B, **geom)


def _prop_operands(H, W, K, T, grads=False):
    """Elements per batch item of every batch-indexed device tensor of a propagate() call."""
    HW = H * W
    ops = {"off_aff": 3 * K * HW, "pred_init": HW, "dep": HW, "confidence": HW, "aff_out": (K + 1) * HW,
           "off_out": 2 * (K + 1) * HW, "conf_out": HW, "pred": HW, "pred_inter": T * HW}
    if grads:  # upstream gradients, the packed gradient, dL/dpred_init, dL/dconf and the workspace (nlspn_prop_bwd.hip)
        ops.update({"grad_pred": HW, "grad_inter": T * HW, "grad_off_aff": 3 * K * HW, "grad_pred_init": HW,
                    "grad_conf": HW, "workspace": (2 + 1 + K + 1) * HW})
    return ops


def _head_operands(C, HW, nout, prologue):
    ops = {"fe1": C * HW, "pred_init": HW, "confidence": HW}
    if prologue:
        ops.update({"dep": HW, "offset": 18 * HW, "aff": 9 * HW, "p0": HW})
    else:
        ops["off_aff"] = nout * HW
    return ops


_P = dict(H=24, W=32, K=8, kh=3, kw=3, T=3)
_HW = 24 * 32
ROWS = [
    # ---- the propagation section: the packed (B, 3K, H, W) head output is the large operand
    _row("prop_f32_s2", "propagate", "off_aff", "f32", "S2", 5, _prop_operands(24, 32, 8, 3), **_P),
    _row("prop_f32_s3", "propagate", "off_aff", "f32", "S3", 5, _prop_operands(24, 32, 8, 3), **_P),
    _row("prop_f16_s3", "propagate", "off_aff", "f16", "S3", 5, _prop_operands(24, 32, 8, 3), **_P),
    # C5's geometry (1 x 17, K = 16) in f16 storage
    _row("prop_f16_k17_s2", "propagate", "off_aff", "f16", "S2", 5, _prop_operands(24, 32, 16, 3),
         H=24, W=32, K=16, kh=1, kw=17, T=3),
    # pred_inter (T, B, 1, H, W) itself crosses S2: an "item" is one (t, b) plane
    _row("prop_inter_s2", "propagate", "pred_inter_plane", "f32", "S2", 5,
         dict(_prop_operands(24, 32, 8, 48), pred_inter_plane=_HW), items_per_batch=48, H=24, W=32, K=8, kh=3, kw=3, T=48),
    # The resident kernel.  Its plan takes at most kResMaxGroups = 64 image groups of at most one part
    # per CU (nlspn_plan.h), so with 256 CUs a 3x3 section's packed input stays below 16384 parts x
    # 2688 px x 96 B = 4.23e9 < 2^32 bytes: the 3x3 row crosses S1 only (two parts per image, 128
    # images per group); the 1x17 f32 row (48 planes per pixel) crosses S2.
    _row("prop_res_s1", "propagate", "off_aff", "f32", "S1", 5, _prop_operands(48, 64, 8, 3),
         H=48, W=64, K=8, kh=3, kw=3, T=3, resident=True),
    _row("prop_res_k17_s2", "propagate", "off_aff", "f32", "S2", 5, _prop_operands(24, 64, 16, 3),
         H=24, W=64, K=16, kh=1, kw=17, T=3, resident=True),
    # ---- the propagation backward through autograd, sparse batch (and dL/dgamma's partials per tile)
    _row("prop_bwd_s2", "propagate backward", "off_aff", "f32", "S2", 5, _prop_operands(24, 32, 8, 3, grads=True), **_P),
    # ---- the stand-alone affinity normalisation
    _row("affnorm_f32_s2", "affinity_normalization", "aff", "f32", "S2", 5, {"aff": 8 * _HW, "out": 9 * _HW}, **_P),
    _row("affnorm_f32_s3", "affinity_normalization", "aff", "f32", "S3", 5, {"aff": 8 * _HW, "out": 9 * _HW}, **_P),
    # (f16: 2^31 elements are 2^32 bytes, one row crosses both)
    _row("affnorm_f16_s3", "affinity_normalization", "aff", "f16", "S3", 5, {"aff": 8 * _HW, "out": 9 * _HW}, **_P),
    _row("affnorm_bwd_s2", "affinity_normalization backward", "aff", "f32", "S2", 5,
         {"aff": 8 * _HW, "out": 9 * _HW, "grad_out": 9 * _HW, "grad_raw": 8 * _HW, "workspace": _HW}, **_P),
    # ---- the head epilogue: C = 16, nout = 24, one tensor as all four sources; fe1 is the large operand
    _row("heads_fp32_s3", "head_epilogue fp32", "fe1", "f32", "S3", 3, _head_operands(16, _HW, 24, False), H=24, W=32, C=16),
    _row("heads_x3_s2", "head_epilogue bf16x3", "fe1", "f32", "S2", 3, _head_operands(16, _HW, 24, False), H=24, W=32, C=16),
    _row("heads_pro_fp32_s2", "head_epilogue_prologue fp32", "fe1", "f32", "S2", 3, _head_operands(16, _HW, 24, True),
         H=24, W=32, C=16),
    _row("heads_pro_x3_s2", "head_epilogue_prologue bf16x3", "fe1", "f32", "S2", 3, _head_operands(16, _HW, 24, True),
         H=24, W=32, C=16),
    # ---- the S2D front: the (B, 17, H, W) output
    _row("s2d_s2", "s2d_front", "out", "f32", "S2", 3, {"dep": _HW, "out": 17 * _HW}, H=24, W=32),
]
# ---- the GRU-mode layers at inference (hc = 128, 64 x 64 inputs), in the three precisions: the stride-2
# encoder convs (9 -> 16 -> 256 -> 128; large: the (B, 9, 64, 64) input, and with it the (B, 256, 16, 16)
# layer), the ConvGRU cell (large: the (B, 128, 8, 8) state) and the transposed decoder convs with the
# fused normalisation (128 -> 256 -> 16 -> 8 + 1; large: the (B, 9, 64, 64) output).  Item sizes are
# powers of two and k = 3: 2^n items are never a whole number of periods.  Operand sizes are in f32
# elements; the f16 / split-bf16 copies of an activation take at most as many bytes again.
_G = dict(H=64, W=64, hc=128)
for _m in ("fp32", "fp16", "bf16x3"):
    _two = 1 if _m == "fp32" else 2
    ROWS += [
        _row(f"gru_enc_{_m}_s2", f"GruConvs.encode_aff {_m}", "aff", "f32", "S2", 3,
             {"aff": 9 * 4096, "l1": _two * 16 * 1024, "l2": _two * 256 * 256, "l3": _two * 128 * 64}, precision=_m, **_G),
        _row(f"gru_cell_{_m}_s2", f"GruConvs.gru {_m}", "h", "f32", "S2", 3,
             {"h": 8192, "x": 8192, "z": 8192, "rh": 8192, "qx": 8192, "hn": 8192, "h_copy": (_two - 1) * 8192,
              "hn_copy": (_two - 1) * 8192}, precision=_m, **_G),
        _row(f"gru_dec_{_m}_s2", f"GruConvs.decode_aff {_m}", "out", "f32", "S2", 3,
             {"h": _two * 8192, "l1": 256 * 256, "l2": _two * 16 * 1024, "out": 9 * 4096}, precision=_m, **_G),
    ]
# ---- the GRU-mode layers under gradients (native f32): the data gradient of one stride-2 conv (16 -> 32)
# and one stride-2 transposed conv (32 -> 16) through GruConvs.layer on the periodic batch (large: the
# (B, 16, 64, 64) tensor), and the weight / bias gradient entries on the sparse batch (large: l, the
# (B, Cl, 64, 64) tensor of a stride-2 conv role; s is (B, Cs, 32, 32))
_L = 16 * 4096
ROWS += [
    _row("gru_dgrad_conv_s2", "GruConvs.layer conv backward", "x", "f32", "S2", 3,
         {"x": _L, "y": _L // 2, "grad_y": _L // 2, "grad_pre": _L // 2, "grad_x": _L}, H=64, W=64),
    _row("gru_dgrad_convt_s2", "GruConvs.layer transposed conv backward", "y", "f32", "S2", 3,
         {"x": _L // 2, "y": _L, "grad_y": _L, "grad_pre": _L, "grad_x": _L // 2}, H=64, W=64),
    _row("gwgrad_fp32_s2", "nlspn_gconv_wgrad", "l", "f32", "S2", 3, {"l": _L, "s": 32 * 1024}, H=64, W=64, Cs=32, Cl=16),
    _row("gwgrad_bf16x3_s2", "nlspn_gconv_wgrad_bf16x3", "l", "f32", "S2", 3, {"l": 2 * _L, "s": 32 * 1024}, H=64, W=64,
         Cs=32, Cl=32),
    _row("gwgrad_narrow_s2", "nlspn_gconv_wgrad_narrow", "l", "f32", "S2", 3, {"l": _L, "s": 16 * 1024}, H=64, W=64,
         Cs=16, Cl=16),
]
# The same three entries in the transposed-conv role (s the (B, Cs, 32, 32) input, l the (B, Cl, 64, 64)
# output gradient, the bias gradient summed from l: bias_from_large)
ROWS += [dict(_r, name=_r["name"].replace("_s2", "_t_s2"), entry=_r["entry"] + " (bias from large)", bfl=True)
         for _r in ROWS[-3:]]
# ---- the ConvGRU cell under gradients through the raw C ABI, as _GruFn.backward calls it (hc = 128, 8 x 8
# states of 2^13 elements, k = 3).  Autograd's cell keeps a dozen state-sized tensors; each entry alone
# stays under the cap.
#   gates1 / gates2: nlspn_gconv_gru_gates_backward stage 1 (du_q, du_z) and stage 2 (du_r, dh), periodic
#   gru_dgrad_cell_{q,zr}: NLSPN_GC_DG_S1 with two outputs: convq's adjoint (cg 128 -> d(rh), dx), then
#       [convz; convr]'s (cg 256) added into dh and dx in place; periodic; large: the gradient g
#   gwgrad_s1_*: the stride-1 two-source weight gradient (s = du, l0 = r*h or h, l1 = x), sparse
_S = 128 * 64
ROWS += [
    _row("gates1_s2", "nlspn_gconv_gru_gates_backward stage 1", "h", "f32", "S2", 3,
         {"dhn": _S, "z": _S, "q": _S, "h": _S, "duq": _S, "duzr": 2 * _S}, H=8, W=8, stage=1),
    _row("gates2_s2", "nlspn_gconv_gru_gates_backward stage 2", "h", "f32", "S2", 3,
         {"dhn": _S, "z": _S, "r": _S, "h": _S, "drh": _S, "duzr": 2 * _S, "dh": _S}, H=8, W=8, stage=2),
    _row("gru_dgrad_cell_q_s2", "nlspn_gconv_dgrad S1 two outputs", "dx", "f32", "S2", 3,
         {"g": _S, "dx": _S, "dx1": _S}, H=8, W=8, cg=128, add="none"),
    _row("gru_dgrad_cell_zr_s2", "nlspn_gconv_dgrad S1 two outputs, add in place", "g", "f32", "S2", 3,
         {"g": 2 * _S, "dx": _S, "dx1": _S}, H=8, W=8, cg=256, add="alias"),
    _row("gwgrad_s1_fp32_s2", "nlspn_gconv_wgrad stride 1, two sources", "l0", "f32", "S2", 3,
         {"s": _S, "l0": _S, "l1": _S}, H=8, W=8),
    _row("gwgrad_s1_bf16x3_s2", "nlspn_gconv_wgrad_bf16x3 stride 1, two sources", "l0", "f32", "S2", 3,
         {"s": _S, "l0": _S, "l1": _S}, H=8, W=8),
]
# ---- the generic DCN, f32, on the geometry with groups of tests/test_gpu_dcn.py (CASES[1]: C = 4, Cout = 6,
# group 2, deformable group 2, 3x3, 13 x 17 images: the kernels have one build, W % 4 plays no part);
# large: the (B, 36, 13, 17) offsets.  Forward on the periodic batch, backward on the sparse batch.
DCN_CASE = 1
_D = 13 * 17
_DCN_OPS = {"input": 4 * _D, "offset": 36 * _D, "mask": 18 * _D, "out": 6 * _D}
ROWS += [
    _row("dcn_fwd_s2", "modulated_deform_conv_forward", "offset", "f32", "S2", 3, _DCN_OPS, H=13, W=17, vector=False),
    _row("dcn_bwd_s2", "modulated_deform_conv_backward", "offset", "f32", "S2", 3,
         dict(_DCN_OPS, grad_out=6 * _D, grad_input=4 * _D, grad_offset=36 * _D, grad_mask=18 * _D), H=13, W=17, vector=False),
]
ROW = {r["name"]: r for r in ROWS}
assert len(ROW) == len(ROWS)

# C4: KITTI at the global batch, against propagate on its eight chunks of 4
C4 = dict(B=32, H=240, W=1216, K=8, T=18, chunk=4)


def n_items(row):
    """Items of the named operand (B, or T * B planes for pred_inter)."""
    return row["B"] * row["items_per_batch"]


def start_offsets(row, item):
    """(bytes, elements) from the named operand's base to the start of `item`."""
    e = item * row["operands"][row["tensor"]]
    return e * row["es"], e


def crossed_tiers(row):
    """The tiers the named operand crosses with at least two whole items beyond."""
    n = n_items(row)
    out = []
    for t, (lim, unit) in TIERS.items():
        b, e = start_offsets(row, n - 2)
        if (b if unit == "bytes" else e) > lim:
            out.append(t)
    return out


def peak_bytes(row):
    """Device bytes of a row's test at its peak: every operand of the call, the comparator's slab
    temporaries and the compact batch (bounded by one slab more)."""
    return row["B"] * sum(row["operands"].get(k, 0) for k in row["operands"] if k != "pred_inter_plane") * row["es"] \
        + 3 * SLAB_BYTES


def alias_free(item_elems, es, k, n):
    """True when no displacement of DISPLACEMENTS maps an item of an n-item tensor (item_elems
    elements of es bytes) onto the start of an item with the same residue mod k."""
    ib = item_elems * es
    for amount, unit in DISPLACEMENTS:
        d = amount if unit == "bytes" else amount * es
        if d >= n * ib:      # beyond the tensor: no item is displaced onto another
            continue
        if d % ib == 0 and (d // ib) % k == 0:
            return False
    return True


def row_alias_free(row):
    return all(alias_free(e, row["es"], row["k"], row["B"]) for n, e in row["operands"].items() if n != "workspace")


def sparse_items(row):
    """The non-zero items of the sparse batch: 0, the first item starting beyond each tier boundary
    the row crosses, and B - 1 (ascending, distinct)."""
    ib = row["operands"][row["tensor"]] * row["es"]
    items = {0, row["B"] - 1}
    for t in crossed_tiers(row):
        items.add(tier_units(t, row["es"]) // ib + 1)
    return sorted(items)


# ------------------------------------------------------------------ the two constructions
def _bits(x):
    """The same storage as integers (bit-for-bit comparison; NaN payloads included); numpy or torch."""
    if isinstance(x, np.ndarray):
        return x.view({2: np.int16, 4: np.int32, 8: np.int64}[x.dtype.itemsize])
    import torch
    return x.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def fill_periodic(big, compact):
    """big[b] = compact[b mod k] in place (numpy or torch; no full-size temporary)."""
    k, n = compact.shape[0], big.shape[0]
    reps = n // k
    if reps:
        body = big[:reps * k].reshape((reps, k) + tuple(big.shape[1:]))
        body[...] = compact.reshape((1, k) + tuple(compact.shape[1:]))
    if n % k:
        big[reps * k:] = compact[:n % k]
    return big


def first_mismatch(out, compact_out, slab_bytes=SLAB_BYTES):
    """The first item b of `out` (n items along dim 0) whose bits differ from compact_out[b mod k],
    or None; compared in slabs of whole periods (numpy or torch, on the tensor's own device)."""
    k, n = compact_out.shape[0], out.shape[0]
    assert tuple(out.shape[1:]) == tuple(compact_out.shape[1:]) and out.dtype == compact_out.dtype
    item = 1
    for d in out.shape[1:]:
        item *= int(d)
    o, c = _bits(out).reshape(n, item), _bits(compact_out).reshape(1, k, item)
    per = max(1, slab_bytes // (k * item))  # a bool per element
    reps = n // k
    for r0 in range(0, reps, per):
        r1 = min(reps, r0 + per)
        bad = (o[r0 * k:r1 * k].reshape(r1 - r0, k, item) != c).reshape(r1 - r0, k * item).any(1)
        if bool(bad.any()):
            r = r0 + int(bad.nonzero()[0][0] if isinstance(bad, np.ndarray) else bad.nonzero()[0, 0])
            for j in range(k):
                if bool((o[r * k + j] != c[0, j]).any()):
                    return r * k + j
    for b in range(reps * k, n):
        if bool((o[b] != c[0, b - reps * k]).any()):
            return b
    return None


def scatter_sparse(big, items, dense):
    """big (zeros) with dense[i] written at item items[i]."""
    for i, b in enumerate(items):
        big[b] = dense[i]
    return big


def nonzero_outside(t, items):
    """True when any item of `t` outside `items` holds a value other than (+-) 0 (NaN counts); the
    ranges between the listed items are reduced in slabs on the tensor's own device."""
    item = 1
    for d in t.shape[1:]:
        item *= int(d)
    per = max(1, SLAB_BYTES // item)
    lo = 0
    for b in list(items) + [t.shape[0]]:
        for s in range(lo, b, per):
            if bool((t[s:min(b, s + per)] != 0).any()):
                return True
        lo = b + 1
    return False
