"""uint8 sources of the fit on the CPU: the byte table against the correctly rounded quotient, the torch specification on uint8
against today's backend and today's host chain, the bound of tests/fit_refs.py, the wrong stand-ins the uint8 inputs of
tests/fit_u8_refs.py have to catch, and the nodes' rules for uint8 clips."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import fit_refs as R
import fit_u8_refs as U

BF = torch.bfloat16


@pytest.fixture(scope="module")
def fit(pkg):
    return R.fit_module(pkg)


# ----------------------------------------------------------------------------------------------- the table
def test_unit_table_is_the_correctly_rounded_quotient(fit):
    t = fit.U8_UNIT
    assert t.dtype == torch.float32 and t.shape == (256,) and t.device.type == "cpu"
    want = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(t.numpy().view(np.uint32), want.view(np.uint32))
    # and exactly: no neighbouring fp32 value is nearer to i / 255 (no tie exists: 255 * 2^k * odd never halves evenly)
    for i in range(256):
        v = np.float32(t[i].item())
        err = abs(Fraction(float(v)) - Fraction(i, 255))
        for other in (np.nextafter(v, np.float32(2.0)), np.nextafter(v, np.float32(-1.0))):
            assert err < abs(Fraction(float(other)) - Fraction(i, 255)), i
    assert t[0] == 0.0 and t[255] == 1.0
    # what the table is for: the reciprocal is another function of the byte
    mul = torch.arange(256, dtype=torch.float32) * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert int((mul != t).sum()) == 126
    assert int(((mul * 2 - 1).to(BF) != (t * 2 - 1).to(BF)).sum()) == 1


def test_u8_unit_is_the_division_on_the_cpu(fit):
    x = torch.arange(256, dtype=torch.uint8).reshape(4, 64)
    assert torch.equal(fit.u8_unit(x), x.float() / 255.0)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (2, 3, 5, 7, 3), generator=g, dtype=torch.uint8)
    got = fit.u8_unit(x)
    assert got.dtype == torch.float32 and got.shape == x.shape and torch.equal(got, x.float() / 255.0)
    with pytest.raises(ValueError, match="uint8"):
        fit.u8_unit(x.float())


# ----------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=R.GEOMETRY_IDS)
def test_torch_backend_on_uint8(pkg, fit, gi):
    for _, B, T in R.grid([gi]):
        c = U.case(pkg, gi, B, T)
        got = fit.fit_frames(c["src"], c["plan"], "cpu")
        assert got.dtype == BF and got.shape == (B, 3, c["plan"].T_out, c["plan"].H_out, c["plan"].W_out)
        assert torch.equal(got, fit.fit_frames(fit.u8_unit(c["src"]), c["plan"], "cpu")), c["name"]      # today's backend
        assert torch.equal(got, fit.fit_frames(c["src"], c["plan"], "cpu", backend="torch")), c["name"]
        if gi in R.SCALE1:
            assert torch.equal(got, c["today"]), c["name"]
            assert torch.equal(got, R.todays_ingest(U.kept(c["src"].float() / 255, c["plan"]))), c["name"]
        ok, ratio = R.bound_excess(got.double(), c["ref64"], c["e_ref"])
        assert c["e_ref"] > 0 and ok, (c["name"], ratio)


def test_other_dtypes_are_refused(fit):
    p = fit.plan_fit(3, 16, 32, "crop")
    for dt in (torch.float64, torch.float16, torch.int16, torch.int8):
        with pytest.raises(ValueError, match="float32 or uint8"):
            fit.fit_frames(torch.zeros(1, 3, 16, 32, 3, dtype=dt), p, "cpu")
    with pytest.raises(ValueError, match="needs a GPU device"):
        fit.fit_frames(torch.zeros(1, 3, 16, 32, 3, dtype=torch.uint8), p, "cpu", backend="hip")


# ----------------------------------------------------------------------------------------------- wrong stand-ins
@pytest.mark.parametrize("name", list(U.wrong_stand_ins()))
def test_wrong_stand_ins_are_caught(pkg, name):
    f = U.wrong_stand_ins()[name]
    hits = [c["name"] for c in (U.case(pkg, *k) for k in R.grid()) if U.caught(pkg, c, f(c["src"]))]
    print(f"{name}: caught at {len(hits)} of {len(list(R.grid()))} cases")
    assert hits, name
    if name == "multiply by 1 / 255":
        # one byte value tells it apart after the bf16 rounding: only a source with every value present sees it
        assert all(U.case(pkg, gi, B, T)["scale1"] for gi, B, T in R.grid() if U.case(pkg, gi, B, T)["name"] in hits)


def test_the_right_reading_is_not_caught(pkg):
    for k in R.grid():
        c = U.case(pkg, *k)
        assert not U.caught(pkg, c, c["src"].float() / 255.0), c["name"]


# ----------------------------------------------------------------------------------------------- nodes
class _Recorder:
    """Stands where the pipeline stands: keeps the batch it is handed and answers with grey frames of its shape."""
    device = "cpu"
    batch_passes = False

    def set_model_type(self, t):
        self.model_type = t

    def generate_video(self, data_batch, normalize_normal=False, seed=None):
        self.batch = data_batch
        B, _, T, H, W = data_batch["video"].shape
        return np.full((B, T, H, W, 3), 128, dtype=np.uint8)


def test_inverse_node_takes_uint8_with_fit_off(pkg):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    p = _Recorder()
    u8 = U.source_u8(1, 9, 16, 32, seed=7)
    outs = node.run_inverse_pass(p, u8)
    assert len(outs) == 5 and outs[0].shape == (9, 16, 32, 3)
    assert p.batch["video"].dtype == BF and torch.equal(p.batch["video"], R.todays_ingest(u8.float() / 255.0))
    node.run_inverse_pass(p, u8.float() / 255.0)          # the fp32 clip: today's path, the same bits once cast
    assert p.batch["video"].dtype == torch.float32 and torch.equal(p.batch["video"].to(BF), R.todays_ingest(u8.float() / 255.0))
    # a T off 8k + 1 is not this rule's business: the clip passes as it is, for the tokenizer to refuse
    node.run_inverse_pass(p, U.source_u8(1, 10, 16, 32))
    assert p.batch["video"].shape == (1, 3, 10, 16, 32)
    for H, W in ((18, 32), (16, 35)):
        with pytest.raises(ValueError, match="fit = 'crop'"):
            node.run_inverse_pass(p, U.source_u8(1, 9, H, W))


def test_inverse_node_fits_uint8(pkg, fit):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    p = _Recorder()
    u8 = U.source_u8(1, 11, 70, 75, seed=8)
    outs = node.run_inverse_pass(p, u8, fit="crop")
    assert outs[0].shape == (11, 64, 64, 3)
    plan = fit.plan_fit(11, 70, 75, "crop")
    assert torch.equal(p.batch["video"], fit.fit_frames(u8.float() / 255.0, plan, "cpu"))


def test_forward_node_takes_mixed_gbuffers(pkg, fit):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    names = ("depth", "normal", "roughness", "metallic", "base_color")
    env = torch.rand(1, 16, 32, 3)
    for kw, (T, H, W) in ((dict(), (9, 32, 32)), (dict(fit="stretch", fit_height=32, fit_width=32), (10, 40, 36))):
        p = _Recorder()
        u8 = {k: U.source_u8(1, T, H, W, seed=20 + i) for i, k in enumerate(names)}
        mixed = {k: (v if k in ("depth", "metallic") else v.float() / 255.0) for k, v in u8.items()}
        node.run_forward_pass(p, *(mixed[k] for k in names), env, **kw)
        seen = dict(p.batch)
        node.run_forward_pass(p, *(u8[k].float() / 255.0 for k in names), env, **kw)
        for k in names:
            key = k.replace("base_color", "basecolor")
            assert seen[key].dtype == (BF if kw or mixed[k].dtype == torch.uint8 else torch.float32), k
            assert torch.equal(seen[key].to(BF), p.batch[key].to(BF)), k
        if kw:
            plan = fit.plan_fit(T, H, W, "stretch", 32, 32)
            assert torch.equal(seen["depth"], fit.fit_frames(u8["depth"], plan, "cpu"))
    with pytest.raises(ValueError, match="'metallic'.*fit = 'crop'"):        # fit off: a uint8 G-buffer off the grid
        bad = {k: torch.rand(1, 9, 32, 32, 3) for k in names}
        bad["metallic"] = U.source_u8(1, 9, 40, 36)
        node.run_forward_pass(_Recorder(), *(bad[k] for k in names), env)
