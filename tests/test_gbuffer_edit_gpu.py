"""drn_gbuffer_edit_u8 on the GPU, bit for bit against the numpy reference (tests/gbuffer_edit_refs.py) at the smallest shapes
where it can go wrong: both address paths, every broadcast, byte offsets, map subsets, in place and out of place, the value
sweeps; every dst inside guard bands and compared whole, every launch made twice.  Then the entry's refusals, the dispatch, and
Cosmos1Relight with tiny nets against the composition by hand.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import fit_refs as FR
import gbuffer_edit_refs as R
from test_relight_gpu import NAMES, _chain, env, pipe  # noqa: F401  (the tiny pipeline and its light, built once for this module)

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
SWEEP_WIDE, SWEEP_NARROW = 2048 * 256 * 16, 2048 * 256          # pixels one sweep of the capped grid covers


class Placed:
    """arr's bytes `off` bytes past a 256-byte aligned base, between guard bands, every byte around them FILL.  pitch16: the
    frames [b, t] lie a multiple of 16 bytes apart with a gap behind each (the wide path's strides at any frame size)."""

    def __init__(self, gpu, arr, off=0, pitch16=False):
        self.shape, self.off = arr.shape, off
        fb = int(np.prod(arr.shape[2:]))
        self.pitch = (fb + 15) // 16 * 16 + 16 if pitch16 else fb
        inner = [int(np.prod(arr.shape[i + 1:])) for i in range(2, arr.ndim)]
        self.strides = (arr.shape[1] * self.pitch, self.pitch, *inner)
        self.total = GUARD + off + arr.shape[0] * arr.shape[1] * self.pitch + GUARD
        self.buf = torch.from_numpy(self.expect(arr)).to(gpu)
        self.view = torch.as_strided(self.buf, arr.shape, self.strides, GUARD + off)

    def expect(self, arr):
        """The whole buffer as it must read with arr in place."""
        e = np.full(self.total, FILL, np.uint8)
        np.lib.stride_tricks.as_strided(e[GUARD + self.off:], self.shape, self.strides)[...] = arr
        return e


def run_case(pkg, gpu, c, subset=range(5), in_place=False, offs=None, extra_frames=0, normal_at=R.NORMAL, pitch16=False):
    """The maps `subset` of case c through ONE launch, twice: every dst buffer equals guard + reference + guard.  offs: byte
    offsets by role ('src', 'dst', 'layer', 'em', 'im'); extra_frames: the sources are [:, :T] views of clips that much longer."""
    offs = offs or {}
    want = R.ref_edit(c)
    B, T = c["maps"][0].shape[:2]
    for _ in range(2):
        em = None if c["edit_mask"] is None else Placed(gpu, c["edit_mask"], offs.get("em", 0), pitch16).view
        im = None if c["insert_mask"] is None else Placed(gpu, c["insert_mask"], offs.get("im", 0), pitch16).view
        maps, checks = [], []
        for k in subset:
            x = c["maps"][k]
            if extra_frames:
                x = np.concatenate([x, np.full((B, extra_frames) + x.shape[2:], 0x3C, np.uint8)], axis=1)
            s = Placed(gpu, x, offs.get("src", 0), pitch16)
            src = s.view[:, :T]
            if in_place:
                d, dst = s, src
                full = np.concatenate([want[k], x[:, T:]], axis=1)                       # frames behind the view are not touched
            else:
                d = Placed(gpu, np.full_like(c["maps"][k], 0x5A), offs.get("dst", 0), pitch16)
                dst, full = d.view, want[k]
            L = None if c["layers"][k] is None else Placed(gpu, c["layers"][k], offs.get("layer", 0), pitch16).view
            maps.append((src, dst, L, c["gain"][k], c["offset"][k], k == normal_at))
            checks.append((k, d, d.expect(full)))
        pkg.native.gbuffer_edit_u8(maps, em, im)
        torch.cuda.synchronize()
        for k, d, exp in checks:
            assert np.array_equal(d.buf.cpu().numpy(), exp), (R.MAPS[k], in_place, offs)


BROADCASTS = {"neither": ((2, 3), (2, 3)), "T": ((2, 1), (2, 1)), "B": ((1, 3), (1, 3)), "both": ((1, 1), (1, 1)),
              "masks_only": ((1, 1), (2, 3)), "layers_only": ((2, 3), (1, 1))}


@pytest.mark.parametrize("path", ("wide", "narrow"))
@pytest.mark.parametrize("px", (1, 5, 15, 16, 17, 257))
def test_shapes_and_broadcasts(pkg, gpu, px, path):
    """B = 2, T = 3, five maps with layers on two of them, masks and layers broadcast in T, in B, in both and in neither."""
    kw = dict(pitch16=True) if path == "wide" else dict(offs={"src": 1, "dst": 1})     # wide: frames a multiple of 16 bytes apart
    for i, (name, (mask_bt, lay_bt)) in enumerate(BROADCASTS.items()):
        c = R.make(100 + px + i, 2, 3, 1, px, mask_bt, mask_bt, lay_bt, layers=(0, 3))
        run_case(pkg, gpu, c, in_place=bool(i & 1), **kw)
    c = R.make(200 + px, 1, 2, 1, px, (1, 2), (1, 1), (1, 2), layers=range(5))          # B = 1, T = 2, five layers
    run_case(pkg, gpu, c, in_place=True, **kw)
    run_case(pkg, gpu, c, in_place=False, **kw)
    one = R.make(250 + px, 1, 1, 1, px, (1, 1), (1, 1), (1, 1), layers=(0, 3))          # B = T = 1: no stride counts
    run_case(pkg, gpu, one, in_place=True, offs=kw.get("offs"))


@pytest.mark.parametrize("path", ("wide", "narrow"))
def test_a_size_past_one_sweep_of_the_capped_grid(pkg, gpu, path):
    px = SWEEP_WIDE + 16 * 3 + 5 if path == "wide" else SWEEP_NARROW + 7
    c = R.make(300, 1, 1, 1, px, (1, 1), (1, 1), (1, 1), layers=(0,))
    run_case(pkg, gpu, c, subset=(0,), in_place=True, offs={} if path == "wide" else {"src": 3})


def test_a_batch_strided_source(pkg, gpu):
    """The node's [:, :keep] views: the clips lie T + 2 frames apart; in place the two frames behind every view keep their bytes."""
    for px in (16, 37):
        c = R.make(310 + px, 2, 3, 1, px, (2, 3), (2, 1), (1, 3), layers=(1, 3))
        for pitch16 in (False, True):
            run_case(pkg, gpu, c, in_place=True, extra_frames=2, pitch16=pitch16)
            run_case(pkg, gpu, c, in_place=False, extra_frames=2, pitch16=pitch16)


def test_every_tensor_alone_off_the_16_byte_grid(pkg, gpu):
    c = R.make(320, 1, 2, 1, 257, (1, 2), (1, 2), (1, 2), layers=(0, 3))
    run_case(pkg, gpu, c, offs={})                                                     # all on the grid
    for role in ("src", "dst", "layer", "em", "im"):
        for off in (1, 2, 3):
            run_case(pkg, gpu, c, in_place=False, offs={role: off})
    for off in (1, 2, 3):
        run_case(pkg, gpu, c, in_place=True, offs={"src": off})


def test_map_subsets(pkg, gpu):
    c = R.make(330, 2, 2, 3, 19, (2, 2), (2, 2), (2, 2), layers=(1, 3))
    for subset in ((2,), (0, 1, 2, 3, 4), (1, 3), (3,), (4, 0)):
        for in_place in (False, True):
            run_case(pkg, gpu, c, subset=subset, in_place=in_place)
    # an insert mask handed in beside maps that have no layer: not read
    run_case(pkg, gpu, c, subset=(0, 2), in_place=True)
    # a map flagged normal without a layer is never renormalised
    run_case(pkg, gpu, c, subset=(0,), normal_at=0)


@pytest.mark.parametrize("name", ("affine_sweep", "blend_pairs", "normals", "high_bytes", "normal_layer_only"))
def test_value_sweeps(pkg, gpu, name):
    """All 256 bytes under the affines that show a fused one; all 65 536 (y, L) pairs under 16 mask values; normal layers on the
    axes, equal, opposite and nearly opposite to the scene's normal."""
    c = R.CASES[name]()
    touched = [k for k in range(5) if c["layers"][k] is not None or c["gain"][k] != [1.0] * 3 or c["offset"][k] != [0.0] * 3]
    run_case(pkg, gpu, c, subset=touched, in_place=name != "blend_pairs")


def test_edit_gbuffers_takes_the_kernel_and_equals_the_specification(pkg, gpu):
    E = R.edit_module(pkg)
    c = R.make(340, 2, 3, 6, 40, (2, 1), (1, 3), (2, 3), layers=(0, 3, 4))
    t = lambda a: None if a is None else torch.from_numpy(a)
    edit = E.GBufferEdit(c["gain"], c["offset"], t(c["edit_mask"]), [t(l) for l in c["layers"]], t(c["insert_mask"]))
    want = R.ref_edit(c)
    spec = E.edit_gbuffers([t(m).to(gpu) for m in c["maps"]], edit, backend="torch")
    maps = [t(m).to(gpu) for m in c["maps"]]
    got = E.edit_gbuffers(maps, edit)                                                 # auto: the kernel, in place
    for k in range(5):
        assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), want[k]) and torch.equal(spec[k], got[k]), R.MAPS[k]
        assert got[k].data_ptr() == maps[k].data_ptr()
    with pytest.raises(ValueError, match="needs GPU tensors"):
        E.edit_gbuffers([t(m) for m in c["maps"]], edit, backend="hip")


def test_the_entry_refuses(pkg, gpu):
    N = pkg.native
    lib = N.load_library()
    px, B, T = 64, 2, 2
    frame = px * 3
    bufs = [torch.zeros(B * T * frame + 64, dtype=torch.uint8, device=gpu) for _ in range(8)]
    em, im = bufs[6], bufs[7]

    def call(change=None, n=2, B=B, T=T, px=px, em=em.data_ptr(), im=im.data_ptr()):
        tab = (N.GbufferEditMap * 6)()
        for k in range(6):
            e = tab[k]
            e.src, e.dst = bufs[k % 3].data_ptr(), bufs[3 + k % 3].data_ptr()
            e.src_bs = e.dst_bs = T * frame
            e.src_ts = e.dst_ts = frame
            for ch in range(3):
                e.gain[ch], e.offset[ch] = 0.5, 3.0
        tab[0].layer, tab[0].layer_bs, tab[0].layer_ts = bufs[2].data_ptr(), T * frame, frame
        tab[1].src = bufs[1].data_ptr()
        if change:
            change(tab)
        return lib.drn_gbuffer_edit_u8(tab, n, em, T * px, px, im, T * px, px, B, T, px, None)

    def setter(k, **kw):
        def f(tab):
            for name, v in kw.items():
                if isinstance(v, tuple):
                    getattr(tab[k], name)[v[0]] = v[1]
                else:
                    setattr(tab[k], name, v)
        return f

    assert call() == 0
    torch.cuda.synchronize()
    assert call(px=0) == 0                                                             # zero pixels: DRN_OK, nothing launched
    EINVAL = -1
    assert lib.drn_gbuffer_edit_u8(None, 2, None, 0, 0, None, 0, 0, B, T, px, None) == EINVAL
    refusals = {
        "null src": setter(1, src=None), "null dst": setter(0, dst=None), "n_maps 0": dict(n=0), "n_maps 6": dict(n=6),
        "B 0": dict(B=0), "T 0": dict(T=0), "pixels -1": dict(px=-1), "a layer without the insert mask": dict(im=None),
        "dst inside the edit mask": setter(1, dst=em.data_ptr() + 16), "dst inside the insert mask": setter(1, dst=im.data_ptr()),
        "dst inside a layer": setter(1, dst=bufs[2].data_ptr() + frame), "dst inside another map's src": setter(1, dst=bufs[0].data_ptr() + 3),
        "dst inside another map's dst": setter(1, dst=bufs[3].data_ptr() + frame), "dst its own src, moved": setter(1, dst=bufs[1].data_ptr() + frame),
        "NaN gain": setter(0, gain=(1, float("nan"))), "inf offset": setter(1, offset=(2, float("inf"))),
    }
    for what, r in refusals.items():
        rc = call(**r) if isinstance(r, dict) else call(r)
        assert rc == EINVAL, what
    torch.cuda.synchronize()
    assert ctypes.sizeof(N.GbufferEditMap) == lib.drn_gbuffer_edit_map_bytes()


# ----------------------------------------------------------------------------------------------- the node, tiny nets
def _node_inputs(T, H, W, seed=50):
    g = torch.Generator().manual_seed(seed)
    em = (torch.rand(1, T, H, W, generator=g) * 1.6 - 0.3).clamp(0, 1)
    im = (torch.rand(1, 1, H, W, generator=g) * 1.6 - 0.3).clamp(0, 1)
    base = torch.rand(1, 1, H, W, 3, generator=g)
    nrm = torch.rand(1, T, H, W, 3, generator=g)
    kw = dict(edit_mask=em[0], edit_base_color_tint=0x80FF40, edit_metallic_gain=0.0, edit_metallic_offset=1.0, edit_roughness_gain=1.7,
              edit_roughness_offset=-0.05, insert_mask=im[0, 0], insert_base_color=base[0], insert_normal=nrm)
    return kw


def test_the_default_relight_call_is_today_s(pkg, gpu, pipe, env):
    T, H, W = 9, 64, 64
    image = FR.source(1, T, H, W, seed=4)
    node = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    opt = node.INPUT_TYPES()["optional"]
    defaults = {k: opt[k][1].get("default") for k in opt if k.startswith(("edit_", "insert_"))}
    assert len(defaults) == 14
    got = node.run_relight(pipe, pipe, image, env, seed=3, env_spin=90.0, **defaults)
    want = _chain(pkg, pipe, image, env, {}, dict(env_spin=90.0, fit="crop"))
    for n, a, b in zip(("image",) + NAMES, got, want):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("mode", ("fit_off", "stretch_restore"))
def test_an_edited_relight_is_the_composition_by_hand(pkg, gpu, pipe, env, mode):
    """The inverse node, then edit_gbuffers with backend='torch' on the host, then the forward node; with fit = 'stretch' and
    fit_restore the masks and layers arrive at the source's size and everything comes back through the way back."""
    E, fit = R.edit_module(pkg), FR.fit_module(pkg)
    T, (H, W) = 9, (64, 64) if mode == "fit_off" else (40, 36)
    fkw = {} if mode == "fit_off" else dict(fit="stretch")
    image = FR.source(1, T, H, W, seed=6)
    kw = _node_inputs(T, H, W)
    node = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()
    got = node.run_relight(pipe, pipe, image, env, seed=3, env_spin=45.0, fit_restore=mode != "fit_off", **fkw, **kw)
    # by hand
    g = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(pipe, image, seed=3, **fkw)
    Hm, Wm = g[0].shape[1:3]
    u8 = [(o * 255.0).round().to(torch.uint8).reshape(1, T, Hm, Wm, 3) for o in g]
    edit = E.build_edit(pkg.nodes.standardize_to_5d, clips=1, **kw)
    plan = None if mode == "fit_off" else fit.plan_fit(T, H, W, "stretch")
    E.check_edit(edit, (1, T, Hm, Wm), source_hw=(H, W))
    fe = E.fit_edit(edit, plan, gpu)                    # the fit's tables on the device, as the node applies them (CPU file: by hand)
    fe = E.GBufferEdit(fe.gain, fe.offset, fe.edit_mask.cpu(), [None if l is None else l.cpu() for l in fe.layers], fe.insert_mask.cpu())
    edited = E.edit_gbuffers(u8, fe, backend="torch")
    assert sum(not torch.equal(a, b) for a, b in zip(edited, u8)) == 4                  # depth alone is untouched
    g5 = dict(zip(NAMES, (e.float() / 255.0 for e in edited)))
    (relit,) = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]().run_forward_pass(
        pipe, g5["depth"], g5["normal"], g5["roughness"], g5["metallic"], g5["base_color"], env, seed=3, env_spin=45.0, fit="crop")
    small = [(relit * 255.0).round().to(torch.uint8)] + list(edited)
    if mode == "fit_off":
        want = [s.float() / 255.0 for s in small]
    else:
        rplan = fit.plan_restore(plan)
        want = [fit.restore_frames(s.to(gpu), rplan).cpu().float() / 255.0 for s in small]
    for n, a, b in zip(("image",) + NAMES, got, want):
        assert torch.equal(a.reshape(b.shape), b), n
