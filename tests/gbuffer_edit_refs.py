"""Relight edits: a numpy reference written independently of gbuffer_edit.py's torch specification, the case grid, and the wrong
stand-ins - each a plausible mistake of a kernel or a specification - with the named case that must catch it
(tests/test_gbuffer_edit_cpu.py proves that each does).  numpy's float32 operators round every operation on its own and its
float32 division is the correctly rounded one, so this file needs no table from the package."""
import numpy as np

F = np.float32
MAPS = ("basecolor", "metallic", "roughness", "normal", "depth")
NORMAL = 3
UNIT = np.arange(256, dtype=F) / F(255.0)                    # unit(i): the correctly rounded i / 255


def edit_module(pkg):
    return pkg.gbuffer_edit


# ----------------------------------------------------------------------------------------------- the reference
def ref_affine(x, g, o, wrong=None):
    xf = x.view(np.int8).astype(F) if wrong == "signed_bytes" else x.astype(F)
    g, o = np.asarray(g, dtype=F), np.asarray(o, dtype=F)
    if wrong == "fused_affine":
        a = (g.astype(np.float64) * xf.astype(np.float64) + o.astype(np.float64)).astype(F)       # one rounding
    else:
        m = g * xf
        a = m + o
    a = np.clip(a, F(0), F(255))
    return (a if wrong == "truncation" else np.rint(a)).astype(np.uint8)


def _weights(m, shape, wrong=None):
    """The mask [b, t, H, W] as fp32 weights broadcast to shape = [B, T, H, W, 3]."""
    B, T, H, W, _ = shape
    if wrong == "mask_frame0":
        m = m[:, :1]
    if wrong == "mask_batch0":
        m = m[:1]
    w = (m.astype(F) / F(256.0)) if wrong == "m_over_256" else UNIT[m]
    w = np.broadcast_to(w, (B, T, H, W))
    if wrong == "mask_per_byte":                             # byte j of a frame weighed by mask byte j (wrapped), not j / 3
        return np.concatenate([w.reshape(B, T, H * W)] * 3, axis=2).reshape(shape)
    return np.broadcast_to(w[..., None], shape)


def ref_blend(a, b, m, wrong=None):
    fa = a.astype(F)
    d = b.astype(F) - fa
    v = fa + _weights(m, a.shape, wrong) * d
    return (v if wrong == "truncation" else np.rint(v)).astype(np.uint8)


def ref_normal(z):
    s = UNIT[z] * F(2.0) - F(1.0)
    l2 = (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2]
    l = np.sqrt(l2.astype(np.float64)).astype(F)            # the correctly rounded fp32 root (no double-rounding case for a root)
    d = np.maximum(l, F(1e-6))
    n = s / d[..., None]
    return np.rint(np.clip((n + F(1.0)) * F(127.5), F(0), F(255))).astype(np.uint8)


def ref_map(x, g, o, em, L, im, is_normal, wrong=None):
    """One map [B, T, H, W, 3] under its affine (g, o per channel), the edit mask (None = 255), its layer (None = none) and the
    matte."""
    def affine(v):
        e = ref_affine(v, g, o, wrong)
        return e if em is None else ref_blend(v, e, em, wrong)

    def insert(v):
        if L is None:
            return v
        lay = np.broadcast_to(L, v.shape)
        if wrong == "layer_real_stride" and (L.shape[0] < v.shape[0] or L.shape[1] < v.shape[1]):
            # a broadcast layer read with the maps' strides: every frame behind the first reads other bytes
            lay = np.stack([np.roll(lay.reshape(-1, *v.shape[2:])[f], f, axis=1) for f in range(v.shape[0] * v.shape[1])]).reshape(v.shape)
        if wrong == "reversed_layer_channels":
            lay = lay[..., ::-1]
        mask = em if wrong == "edit_mask_on_insert" and em is not None else im
        z = ref_blend(v, lay, mask, wrong)
        if is_normal and wrong != "normal_not_renormalised":
            hit = np.broadcast_to((im != 0)[..., None], v.shape)
            if wrong == "normal_renormalised_everywhere":
                hit = np.ones_like(hit)
            z = np.where(hit, ref_normal(z), z)
        return z

    return affine(insert(x)) if wrong == "insert_before_affine" else insert(affine(x))


def ref_edit(case, wrong=None):
    """The five maps of a case -> the five edited maps."""
    out, last_layer = [], None
    for k, x in enumerate(case["maps"]):
        g, o, L = case["gain"][k], case["offset"][k], case["layers"][k]
        if wrong == "affine_on_normal" and k == NORMAL:
            g, o = case["gain"][k - 1], case["offset"][k - 1]          # the row of the map in front
        if wrong == "stale_layer":                                      # a map without a layer blended with the last layer seen
            if L is None:
                L = last_layer
            else:
                last_layer = L
        out.append(ref_map(x, g, o, case["edit_mask"], L, case["insert_mask"], k == NORMAL, wrong))
    return out


# ----------------------------------------------------------------------------------------------- the cases
MASK_VALUES = (0, 1, 2, 3, 64, 85, 100, 127, 128, 129, 170, 200, 253, 254, 255, 17)      # 16, with 0 1 127 128 254 255


def mask(rng, b, t, H, W):
    """Bytes with plenty of 0 and 255, the rest anything."""
    m = rng.integers(0, 256, (b, t, H, W), dtype=np.uint8)
    kind = rng.integers(0, 4, (b, t, H, W))
    m[kind == 0] = 0
    m[kind == 1] = 255
    return m


def make(seed, B, T, H, W, em_bt=None, im_bt=None, lay_bt=None, layers=(), affine=True):
    """A random case: em_bt / im_bt / lay_bt = (b, t) of the masks and layers (None: no mask; b, t in {1, B} x {1, T}); layers: the
    maps that get one."""
    rng = np.random.default_rng(seed)
    maps = [rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8) for _ in MAPS]
    gain = [[1.0] * 3 for _ in MAPS]
    offset = [[0.0] * 3 for _ in MAPS]
    if affine:
        gain[0], offset[0] = [0.3, 1.7, 1.0], [7.3, 7.3, -20.0]
        gain[1], offset[1] = [0.0] * 3, [255.0] * 3                       # a constant: fully metallic
        gain[2], offset[2] = [1.7, 0.7, 8.0], [7.3, -3.1, -255.0]
        gain[4], offset[4] = [0.3] * 3, [0.0] * 3
    return {"maps": maps, "gain": gain, "offset": offset,
            "edit_mask": None if em_bt is None else mask(rng, *em_bt, H, W),
            "insert_mask": None if im_bt is None else mask(rng, *im_bt, H, W),
            "layers": [rng.integers(0, 256, (*lay_bt, H, W, 3), dtype=np.uint8) if k in layers else None for k in range(5)]}


def case_affine_sweep():
    """All 256 bytes under the affines that show a fused one (and under every other row of `make`), the mask 255 or absent."""
    c = make(1, 1, 1, 3, 256, affine=True)
    for k in range(5):
        c["maps"][k][...] = np.arange(256, dtype=np.uint8)[None, None, None, :, None]
    return c


def case_blend_pairs():
    """All 65 536 (y, L) pairs under 16 mask values: frame t has the mask MASK_VALUES[t] everywhere, y = the row, L = the column."""
    c = make(2, 1, 16, 256, 256, affine=False)
    y = np.arange(256, dtype=np.uint8)
    c["maps"][1][...] = y[None, None, :, None, None]
    c["layers"][1] = np.broadcast_to(y[None, None, None, :, None], (1, 1, 256, 256, 3)).copy()
    c["insert_mask"] = np.broadcast_to(np.array(MASK_VALUES, dtype=np.uint8)[None, :, None, None], (1, 16, 256, 256)).copy()
    return c


def encode(v):
    v = np.asarray(v, dtype=np.float64)
    return np.rint(np.clip((v + 1.0) * 127.5, 0, 255)).astype(np.uint8)


def case_normals():
    """Normal layers on the axes, equal to the scene's normal, opposite to it (the half-way mattes land on the shortest vectors a
    byte triple decodes to) and nearly opposite, each under the mattes 0, 1, 127, 128, 129 and 255; the other maps untouched."""
    scene = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.0, 0.8), (0.577, 0.577, 0.577)]
    pairs = []
    for s in scene:
        sb = encode(s)
        opposite = (255 - sb.astype(np.int32)).astype(np.uint8)
        near = opposite.copy()
        near[0] = near[0] + 1 if near[0] < 255 else 254
        for L in [encode(a) for a in scene[:6]] + [sb, opposite, near]:
            pairs.append((sb, L))
    mattes = (0, 1, 127, 128, 129, 255)
    W = len(pairs)
    c = make(3, 1, 1, len(mattes), W, affine=False)
    c["maps"][NORMAL][0, 0] = np.stack([p[0] for p in pairs])[None]
    c["layers"][NORMAL] = np.broadcast_to(np.stack([p[1] for p in pairs])[None, None, None], (1, 1, len(mattes), W, 3)).copy()
    c["insert_mask"] = np.broadcast_to(np.array(mattes, dtype=np.uint8)[None, None, :, None], (1, 1, len(mattes), W)).copy()
    return c


B, T, H, W = 2, 3, 5, 7
CASES = {
    "affine_sweep": case_affine_sweep,
    "blend_pairs": case_blend_pairs,
    "normals": case_normals,
    "broadcast_none": lambda: make(10, B, T, H, W, (B, T), (B, T), (B, T), layers=range(5)),
    "broadcast_T": lambda: make(11, B, T, H, W, (B, 1), (B, 1), (B, 1), layers=range(5)),
    "broadcast_B": lambda: make(12, B, T, H, W, (1, T), (1, T), (1, T), layers=range(5)),
    "broadcast_both": lambda: make(13, B, T, H, W, (1, 1), (1, 1), (1, 1), layers=range(5)),
    "masks_per_frame_layers_broadcast": lambda: make(14, B, T, H, W, (B, T), (B, T), (1, 1), layers=(0, 3)),
    "two_layers_of_five": lambda: make(15, B, T, H, W, (B, T), (B, T), (B, T), layers=(0, 2)),
    "normal_layer_only": lambda: make(16, B, T, H, W, None, (B, T), (B, T), layers=(3,), affine=False),
    "affine_no_mask": lambda: make(17, B, T, H, W, None, None, None),
    "affine_under_mask": lambda: make(18, B, T, H, W, (B, T), None, None),
    "layers_no_affine": lambda: make(19, B, T, H, W, None, (B, T), (B, T), layers=range(5), affine=False),
    "high_bytes": lambda: _high(make(20, 1, 1, 4, 64, (1, 1), (1, 1), (1, 1), layers=range(5))),
}


def _high(c):
    for k in range(5):
        c["maps"][k] |= 0x80                                             # every byte 128..255: what signed bytes get wrong
    return c


# the wrong stand-ins, each with the case that catches it
STAND_INS = {
    "fused_affine": "affine_sweep",
    "truncation": "affine_sweep",
    "m_over_256": "blend_pairs",
    "signed_bytes": "high_bytes",
    "mask_per_byte": "broadcast_none",
    "mask_frame0": "broadcast_B",
    "mask_batch0": "broadcast_T",
    "layer_real_stride": "masks_per_frame_layers_broadcast",
    "insert_before_affine": "broadcast_none",
    "edit_mask_on_insert": "broadcast_none",
    "reversed_layer_channels": "broadcast_none",
    "normal_not_renormalised": "normals",
    "normal_renormalised_everywhere": "normal_layer_only",
    "affine_on_normal": "affine_no_mask",
    "stale_layer": "two_layers_of_five",
}
