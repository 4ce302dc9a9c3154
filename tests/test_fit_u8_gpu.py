"""drn_fit_frames_u8 (the uint8 instantiation of csrc/fit.hip's kernel) on the GPU: bit for bit the fp32 kernel on u8_unit(src) at
every geometry, within the float64 bound of tests/fit_refs.py (whose uint8 inputs tests/test_fit_u8_cpu.py shows to catch the wrong
stand-ins), bit for bit today's host chain at scale 1, a source at every byte alignment, spans beyond the raw buffer, a tile cut
into one chunk per row, its argument checks, and fit.fit_frames on uint8."""
import numpy as np
import pytest
import torch

import fit_refs as R
import fit_u8_refs as U

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD, SENTINEL = 64, 0xA5          # 64 bytes keep the guarded output 16-byte aligned
DRN_EINVAL = -1


def _launch(pkg, gpu, src, plan, fn="fit_frames_u8"):
    """The kernel into a guard-banded buffer, issued twice (a rerun over its own output changes nothing) -> the result on the CPU;
    the guard bands are checked here."""
    B = src.shape[0]
    shape = (B, 3, plan.t_idx.shape[0], plan.y_lo_n.shape[0], plan.x_lo_n.shape[0])
    n = 2 * int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:GUARD + n].view(BF).view(shape)
    for _ in range(2):
        getattr(pkg.native, fn)(src, plan.t_idx, plan.y_lo_n, plan.y_w, plan.x_lo_n, plan.x_w, out=out)
    host = buf.cpu()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "wrote outside its output"
    return host[GUARD:GUARD + n].view(BF).view(shape)


def _at_offset(src, off, gpu):
    """The bytes of `src` at byte offset `off` (mod 4) inside a sentinel-filled allocation."""
    n = src.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 4 == 0
    buf[GUARD + off:GUARD + off + n] = src.reshape(-1).to(gpu)
    view = buf[GUARD + off:GUARD + off + n].view(src.shape)
    assert view.data_ptr() % 4 == off and view.is_contiguous()
    return view


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=R.GEOMETRY_IDS)
def test_kernel_equals_the_fp32_kernel_and_meets_the_bound(pkg, gpu, gi):
    fit = R.fit_module(pkg)
    worst = 0.0
    for _, B, T in R.grid([gi]):
        c = U.case(pkg, gi, B, T)
        p = c["plan"]
        src = c["src"].to(gpu)
        got = _launch(pkg, gpu, src, p)
        unit = fit.u8_unit(src)
        assert torch.equal(unit.cpu(), c["src"].float() / 255.0)                  # the lookup gives the CPU's bits on the device
        assert torch.equal(got, _launch(pkg, gpu, unit, p, fn="fit_frames")), c["name"]      # the unchanged fp32 kernel
        ok, ratio = R.bound_excess(got.double(), c["ref64"], c["e_ref"])
        print(f"fit-u8 parity {c['name']}: E_ref {c['e_ref']:.3e}, max((|hip - ref64| - 0.5 ulp)+ / E_ref) = {ratio:.3f}")
        assert ok, (c["name"], ratio)
        worst = max(worst, ratio)
        if gi in R.SCALE1:
            assert torch.equal(got, c["today"]), c["name"]                        # (u8.float() / 255).permute * 2 - 1 -> bf16
            assert torch.equal(got, fit.fit_frames(c["src"], p, gpu, backend="torch").cpu()), c["name"]
            assert torch.equal(got, fit.fit_frames(c["src"], p, gpu).cpu()), c["name"]            # auto = the kernel on a GPU
    print(f"fit-u8 parity {R.GEOMETRY_IDS[gi]}: worst ratio {worst:.3f} (bound {R.M_BOUND})")


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=R.GEOMETRY_IDS)
def test_kernel_source_at_every_byte_alignment(pkg, gpu, gi):
    c = U.case(pkg, gi, 2, 3)
    base = _launch(pkg, gpu, c["src"].to(gpu), c["plan"])
    for off in range(4):
        assert torch.equal(_launch(pkg, gpu, _at_offset(c["src"], off, gpu), c["plan"]), base), off


@pytest.mark.parametrize("Ws", (900, 2100))
def test_kernel_spans_beyond_the_raw_buffer(pkg, gpu, Ws):
    """Tables no resize produces: a tile whose columns read both ends of a long row.  900 columns: two source rows per raw pass;
    2100: the span does not fit and is read directly.  Still the fp32 kernel's bits."""
    fit = R.fit_module(pkg)
    Hs, Hd, Wd = 5, 16, 32
    src = U.source_u8(2, 2, Hs, Ws, seed=31)
    x = torch.arange(Wd)
    plan = type("P", (), {})()
    plan.t_idx = torch.tensor([1, 0, 1], dtype=torch.int32)
    plan.y_lo_n = torch.stack([torch.arange(Hd) % (Hs - 1), torch.full((Hd,), 2)], 1).to(torch.int32)
    plan.y_w = torch.tensor([[0.25, 0.75]], dtype=torch.float32).repeat(Hd, 1)
    plan.x_lo_n = torch.stack([torch.where(x % 2 == 0, x, Ws - 3 - x), torch.full((Wd,), 3)], 1).to(torch.int32)
    plan.x_w = torch.tensor([[0.5, 0.125, 0.375]], dtype=torch.float32).repeat(Wd, 1)
    for off in (0, 3):
        dev = _at_offset(src, off, gpu)
        assert torch.equal(_launch(pkg, gpu, dev, plan), _launch(pkg, gpu, fit.u8_unit(dev), plan, fn="fit_frames"))


def test_scattered_row_taps_cut_a_tile_into_one_chunk_per_row(pkg, gpu):
    """No two consecutive output rows fit the stage together (fit_refs.scattered_rows): one chunk, and one raw pass, per output
    row.  Still the fp32 kernel's bits."""
    fit = R.fit_module(pkg)
    plan = R.scattered_rows()[0]
    src = U.source_u8(1, 2, 120, 40, seed=32)
    for off in (0, 3):
        dev = _at_offset(src, off, gpu)
        assert torch.equal(_launch(pkg, gpu, dev, plan), _launch(pkg, gpu, fit.u8_unit(dev), plan, fn="fit_frames"))


def test_kernel_argument_checks(pkg, gpu):
    lib = pkg.native.load_library()
    c = U.case(pkg, 0, 1, 3)
    p = c["plan"]
    src = c["src"].to(gpu)
    tabs = [t.to(gpu) for t in (p.t_idx, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)]
    n = 2 * 3 * p.T_out * p.H_out * p.W_out
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:].data_ptr()
    assert out % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    base = dict(src=src.data_ptr(), dst=out, B=1, Ts=3, Hs=p.H, Ws=p.W, Td=p.T_out, Hd=p.H_out, Wd=p.W_out,
                t_idx=tabs[0].data_ptr(), y_lo_n=tabs[1].data_ptr(), y_w=tabs[2].data_ptr(), Ky=p.y_w.shape[1],
                x_lo_n=tabs[3].data_ptr(), x_w=tabs[4].data_ptr(), Kx=p.x_w.shape[1])

    def call(**kw):
        a = dict(base, **kw)
        return lib.drn_fit_frames_u8(a["src"], a["dst"], a["B"], a["Ts"], a["Hs"], a["Ws"], a["Td"], a["Hd"], a["Wd"], a["t_idx"],
                                     a["y_lo_n"], a["y_w"], a["Ky"], a["x_lo_n"], a["x_w"], a["Kx"], stream)
    bad = {f"null {k}": {k: None} for k in ("src", "dst", "t_idx", "y_lo_n", "y_w", "x_lo_n", "x_w")}
    bad.update({f"{k} = 0": {k: 0} for k in ("B", "Ts", "Hs", "Ws", "Td", "Hd", "Wd")})
    bad.update({"B < 0": dict(B=-1), "Ky = 0": dict(Ky=0), "Ky = 33": dict(Ky=33), "Kx = 0": dict(Kx=0), "Kx = 33": dict(Kx=33),
                "Hd = 24": dict(Hd=24), "Wd = 8": dict(Wd=8), "Hd = 17": dict(Hd=17),
                "output of 2^31 elements": dict(B=1 << 14, Td=1 << 8, Hd=16, Wd=16 * 11),            # 3 * 2^22 * 176 > 2^31
                "source of 2^31 bytes": dict(B=1 << 12, Ts=1 << 8, Hs=1 << 8, Ws=1 << 4),             # 3 * 2^32
                "y_w 1 byte off": dict(y_w=tabs[2].data_ptr() + 1), "x_w 2 bytes off": dict(x_w=tabs[4].data_ptr() + 2),
                "t_idx 2 bytes off": dict(t_idx=tabs[0].data_ptr() + 2),
                "dst 8 bytes off": dict(dst=out + 8), "dst 2 bytes off": dict(dst=out + 2)})
    for name, kw in bad.items():
        assert call(**kw) == DRN_EINVAL, name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all(), "a rejected call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all()
    # the wrapper reads the tables where their contents can be read, and takes bytes only
    for name, t in (("y_lo_n", p.y_lo_n.clone()), ("x_lo_n", p.x_lo_n.clone())):
        t[-1, 0] += 40
        kw = dict(t_idx=p.t_idx, y_lo_n=p.y_lo_n, y_w=p.y_w, x_lo_n=p.x_lo_n, x_w=p.x_w)
        kw[name] = t
        with pytest.raises(AssertionError, match="taps outside the source"):
            pkg.native.fit_frames_u8(src, **kw)
    with pytest.raises(AssertionError, match="t_idx outside the clip"):
        pkg.native.fit_frames_u8(src, p.t_idx + 1, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)
    with pytest.raises(AssertionError, match="uint8"):
        pkg.native.fit_frames_u8(src.float(), p.t_idx, p.y_lo_n, p.y_w, p.x_lo_n, p.x_w)


def test_fit_frames_takes_host_and_device_bytes(pkg, gpu):
    fit = R.fit_module(pkg)
    for gi in (3, 5):
        c = U.case(pkg, gi, 2, 10)
        host = fit.fit_frames(c["src"], c["plan"], gpu)
        dev = fit.fit_frames(c["src"].to(gpu), c["plan"], gpu, backend="hip")
        assert host.is_cuda and host.dtype == BF and torch.equal(host, dev)
        assert torch.equal(host, fit.fit_frames(fit.u8_unit(c["src"]), c["plan"], gpu))            # the fp32 path, untouched
    with pytest.raises(ValueError, match="float32 or uint8"):
        fit.fit_frames(c["src"].to(gpu).short(), c["plan"], gpu)
