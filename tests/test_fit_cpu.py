"""fit.py on the CPU: the tap tables against F.interpolate in float64, the plan's rules, the torch specification against today's
ingest and against the bound of tests/fit_refs.py, the wrong stand-ins that bound has to catch, and the nodes' new inputs."""
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fit_refs as R

BF = torch.bfloat16


@pytest.fixture(scope="module")
def fit(pkg):
    return R.fit_module(pkg)


def _dense(lo_n, w, n_in):
    m = torch.zeros(lo_n.shape[0], n_in, dtype=torch.float64)
    for r, (lo, n) in enumerate(lo_n.tolist()):
        m[r, lo:lo + n] = torch.as_tensor(w[r, :n], dtype=torch.float64)
    return m


# ----------------------------------------------------------------------------------------------- tables
def test_tables_equal_interpolate_in_float64(fit):
    g = torch.Generator().manual_seed(3)
    worst, n_cases = 0.0, 0
    for H in range(16, 81):
        W = 16 + (H * 7) % 65
        img = torch.rand(1, 1, H, W, dtype=torch.float64, generator=g)
        for mode in ("crop", "stretch"):
            for fh, fw in ((16, 32), (32, 16), (48, 48), (80, 64), (0, 0)):
                p = fit.plan_fit(1, H, W, mode, fh, fw)
                y_lo_n, y_w = fit.axis_taps(H, p.H_full, p.y0, p.H_out)
                x_lo_n, x_w = fit.axis_taps(W, p.W_full, p.x0, p.W_out)
                for lo_n, w, n_in in ((y_lo_n, y_w, H), (x_lo_n, x_w, W)):
                    lo, n = lo_n[:, 0].astype(np.int64), lo_n[:, 1].astype(np.int64)
                    assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all() and n.max() == w.shape[1]
                    assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-15
                    cols = np.arange(w.shape[1])[None, :]
                    assert (w[cols >= n[:, None]] == 0).all()                               # padding
                    assert (w[np.arange(len(n)), 0] != 0).all() and (w[np.arange(len(n)), n - 1] != 0).all()   # zero taps dropped
                # the plan's fp32 tables are these, rounded
                assert torch.equal(p.y_lo_n, torch.from_numpy(y_lo_n)) and torch.equal(p.y_w, torch.from_numpy(y_w.astype(np.float32)))
                assert torch.equal(p.x_lo_n, torch.from_numpy(x_lo_n)) and torch.equal(p.x_w, torch.from_numpy(x_w.astype(np.float32)))
                got = _dense(y_lo_n, y_w, H) @ img[0, 0] @ _dense(x_lo_n, x_w, W).T
                ref = F.interpolate(img, size=(p.H_full, p.W_full), mode="bilinear", antialias=True, align_corners=False)
                ref = ref[0, 0, p.y0:p.y0 + p.H_out, p.x0:p.x0 + p.W_out]
                worst = max(worst, float((got - ref).abs().max()))
                # the tests' own float64 tables say the same
                mine = R.ref_taps(H, p.H_full, p.y0, p.H_out) @ img[0, 0] @ R.ref_taps(W, p.W_full, p.x0, p.W_out).T
                worst = max(worst, float((mine - ref).abs().max()))
                n_cases += 1
    print(f"tables vs F.interpolate(float64): {n_cases} plans, max abs difference {worst:.2e}")
    assert worst <= 1e-12


def test_scale_one_is_one_tap_of_weight_one(fit):
    lo_n, w = fit.axis_taps(40, 40, 4, 32)
    assert w.shape == (32, 1) and (w == 1.0).all() and (lo_n[:, 0] == np.arange(4, 36)).all() and (lo_n[:, 1] == 1).all()
    # the tap counts the issue quotes: 4 per axis at the 1.875 ratio, 6 at 45 -> 16
    assert fit.axis_taps(1080, 576, 0, 576)[1].shape[1] == 4 and fit.axis_taps(1920, 1024, 0, 1024)[1].shape[1] == 4
    assert fit.axis_taps(45, 16, 0, 16)[1].shape[1] == 6


# ----------------------------------------------------------------------------------------------- plan
def test_plan_properties(fit):
    for H, W in [(h, 16 + (h * 11) % 115) for h in range(16, 131)]:
        for mode in ("crop", "stretch"):
            for fh, fw in ((0, 0), (32, 0), (0, 48), (64, 32), (16, 128)):
                p = fit.plan_fit(9, H, W, mode, fh, fw)
                assert p.H_out % 16 == 0 and p.W_out % 16 == 0 and p.H_out > 0 and p.W_out > 0
                assert p.H_out == (fh or H // 16 * 16) and p.W_out == (fw or W // 16 * 16)
                if not fh:
                    assert H - 16 < p.H_out <= H
                if not fw:
                    assert W - 16 < p.W_out <= W
                assert tuple(p.y_lo_n.shape) == (p.H_out, 2) and tuple(p.x_lo_n.shape) == (p.W_out, 2)
                assert p.y_lo_n.dtype == torch.int32 and p.y_w.dtype == torch.float32 and p.t_idx.dtype == torch.int32
                assert p.y_w.shape[0] == p.H_out and p.x_w.shape[0] == p.W_out
                if mode == "stretch":
                    assert (p.H_full, p.W_full, p.y0, p.x0) == (p.H_out, p.W_out, 0, 0)
                else:
                    assert p.H_full >= p.H_out and p.W_full >= p.W_out                           # covers the target
                    assert p.y0 == (p.H_full - p.H_out) // 2 and p.x0 == (p.W_full - p.W_out) // 2   # centred
                    assert p.H_full == p.H_out or p.W_full == p.W_out or not (fh or fw)          # one side fits exactly
                    if not fh and not fw:
                        assert (p.H_full, p.W_full) == (H, W) and p.y_w.shape[1] == 1 and p.x_w.shape[1] == 1
                    else:
                        s = max(p.H_out / H, p.W_out / W)
                        assert abs(p.H_full - H * s) <= 0.5 + 1e-9 or p.H_full == p.H_out
                        assert abs(p.W_full - W * s) <= 0.5 + 1e-9 or p.W_full == p.W_out
                assert p.identity == (H % 16 == 0 and W % 16 == 0 and (p.H_out, p.W_out) == (H, W))
    p = fit.plan_fit(57, 1080, 1920, "crop")
    assert (p.H_out, p.W_out, p.y0, p.x0) == (1072, 1920, 4, 0) and int(p.y_lo_n[0, 0]) == 4 and int(p.y_lo_n[-1, 0]) == 1075
    p = fit.plan_fit(57, 1080, 1920, "crop", 576, 1024)
    assert (p.H_full, p.W_full, p.y0, p.x0) == (576, 1024, 0, 0) and p.y_w.shape[1] == 4 and p.x_w.shape[1] == 4


def test_plan_time_rule(fit):
    for T in range(1, 41):
        p = fit.plan_fit(T, 32, 32, "crop")
        assert (p.T_out - 1) % 8 == 0 and T <= p.T_out < T + 8 and p.T == T
        assert p.t_idx.tolist() == [min(t, T - 1) for t in range(p.T_out)]
        assert p.identity == ((T - 1) % 8 == 0)
        w = fit.plan_fit(T, 32, 32, "crop", windowed=True)
        assert w.T_out == T and w.t_idx.tolist() == list(range(T)) and w.identity


def test_plan_errors(fit):
    for kw in (dict(height=24), dict(width=40), dict(height=-16), dict(width=-32)):
        with pytest.raises(ValueError, match="multiple of 16"):
            fit.plan_fit(9, 64, 64, "crop", **kw)
    with pytest.raises(ValueError, match="below the model's grid"):
        fit.plan_fit(9, 15, 64, "crop")
    with pytest.raises(ValueError, match="below the model's grid"):
        fit.plan_fit(9, 64, 12, "stretch", height=32)
    assert fit.plan_fit(9, 12, 64, "stretch", height=16).H_out == 16          # a given target may up-sample a small source
    with pytest.raises(ValueError, match="fit mode"):
        fit.plan_fit(9, 64, 64, "letterbox")
    with pytest.raises(ValueError, match="taps"):
        fit.plan_fit(1, 16 * 17, 64, "stretch", height=16)                    # a 17x down-scale: 35 taps
    assert fit.plan_fit(1, 16 * 15, 64, "stretch", height=16).y_w.shape[1] <= 32
    with pytest.raises(ValueError, match="empty clip"):
        fit.plan_fit(0, 64, 64, "crop")


# ----------------------------------------------------------------------------------------------- torch backend
def test_torch_backend_at_scale_one_is_todays_ingest(pkg, fit):
    for gi in R.SCALE1:
        for B in R.BATCHES:
            for T in R.FRAMES:
                c = R.case(pkg, gi, B, T)
                p = c["plan"]
                got = fit.fit_frames(c["src"], p, "cpu")
                frames = c["src"][:, p.t_idx.long(), p.y0:p.y0 + p.H_out, p.x0:p.x0 + p.W_out]
                assert got.dtype == BF and got.is_contiguous() and torch.equal(got, R.todays_ingest(frames)), c["name"]
    c = R.case(pkg, 5, 1, 1)
    assert (c["plan"].y0, c["plan"].x0, c["plan"].H_out, c["plan"].W_out) == (1, 1, 16, 32)       # rows 1..16, columns 1..32


def test_specification_meets_the_bound_at_every_case(pkg, fit):
    for gi, B, T in R.grid():
        c = R.case(pkg, gi, B, T)
        p = c["plan"]
        assert tuple(c["ref64"].shape) == (B, 3, p.T_out, p.H_out, p.W_out) and p.T_out == {1: 1, 3: 9, 9: 9, 10: 17}[T]
        got = fit.fit_frames(c["src"], p, "cpu", backend="torch")
        ok, ratio = R.bound_excess(got.double(), c["ref64"], c["e_ref"])
        assert ok and ratio <= 1.0 + 1e-9, (c["name"], ratio)         # one rounding of a value within E_ref: ratio <= 1 by construction
        # at scale 1 the specification is exact (2v - 1 of a rand() value has no rounding): the bound is the bf16 rounding alone
        assert (c["e_ref"] == 0) if gi in R.SCALE1 else (0 < c["e_ref"] < 1e-5), (c["name"], c["e_ref"])
        ok, _ = R.bound_excess(c["ref64"], c["ref64"], c["e_ref"])
        assert ok


@pytest.mark.parametrize("name", list(R.wrong_stand_ins()))
def test_wrong_stand_in_misses_the_bound(pkg, name):
    f = R.wrong_stand_ins()[name]
    missed = []
    for gi, B, T in R.grid():
        if B != 1:
            continue
        c = R.case(pkg, gi, B, T)
        ok, ratio = R.bound_excess(f(c), c["ref64"], c["e_ref"])
        if not ok:
            missed.append(c["name"])
    print(f"{name}: misses the bound at {len(missed)} cases, first {missed[:2]}")
    assert missed, name


def test_ulp_bf16():
    x = torch.tensor([1.0, 1.5, 0.999, 2.0, -0.75, 0.0, 3e-39], dtype=torch.float64)
    assert R.ulp_bf16(x).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133]


def test_fit_frames_errors(pkg, fit):
    p = fit.plan_fit(3, 18, 35, "crop")
    with pytest.raises(ValueError, match="needs a GPU device"):
        fit.fit_frames(torch.rand(1, 3, 18, 35, 3), p, "cpu", backend="hip")
    with pytest.raises(ValueError, match=r"\[B, T, H, W, 3\]"):
        fit.fit_frames(torch.rand(1, 3, 18, 35, 4), p, "cpu")
    with pytest.raises(ValueError, match="plan was made for"):
        fit.fit_frames(torch.rand(1, 3, 18, 36, 3), p, "cpu")
    with pytest.raises(ValueError, match="unknown backend"):
        fit.fit_frames(torch.rand(1, 3, 18, 35, 3), p, "cpu", backend="triton")


# ----------------------------------------------------------------------------------------------- nodes
@pytest.mark.parametrize("node", ["Cosmos1InverseRenderer", "Cosmos1ForwardRenderer"])
def test_nodes_declare_the_fit_inputs(pkg, node):
    opt = pkg.NODE_CLASS_MAPPINGS[node].INPUT_TYPES()["optional"]
    assert opt["fit"][0] == ["off", "crop", "stretch"] and opt["fit"][1]["default"] == "off"
    assert "not resampled back" in opt["fit"][1]["tooltip"]
    for k in ("fit_height", "fit_width"):
        kind, o = opt[k]
        assert kind == "INT" and o["default"] == 0 and o["min"] == 0 and o["step"] == 16 and o["tooltip"]


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


def _gbuffers(T, H, W):
    return {k: R.source(1, T, H, W, seed=i) for i, k in enumerate(("depth", "normal", "roughness", "metallic", "base_color"))}


def test_forward_node_rescales_the_spin_and_cuts_the_padding(pkg, monkeypatch):
    pe = importlib.import_module(pkg.__name__ + ".preprocess_envmap")
    seen = {}
    real = pe.envmap_conditions

    def recording(env_map, resolution, num_frames, *a, **kw):
        seen.update(resolution=tuple(resolution), num_frames=num_frames, env_spin=kw.get("env_spin"))
        return real(env_map, resolution, num_frames, *a, **kw)
    monkeypatch.setattr(pe, "envmap_conditions", recording)
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    p = _Recorder()
    g = _gbuffers(10, 40, 36)
    env = torch.rand(1, 16, 32, 3)
    (out,) = node.run_forward_pass(p, g["depth"], g["normal"], g["roughness"], g["metallic"], g["base_color"], env,
                                   env_spin=90.0, fit="crop")
    assert out.shape == (1, 10, 32, 32, 3)                                     # cut to the clip's own 10 frames
    assert seen["resolution"] == (32, 32) and seen["num_frames"] == 17
    angles = pe.spin_angles(seen["env_spin"], 17)
    for t in range(10):
        assert math.isclose(angles[t], math.radians(90.0) * t / 10, rel_tol=1e-12, abs_tol=1e-15)
    fit = R.fit_module(pkg)
    plan = fit.plan_fit(10, 40, 36, "crop")
    assert torch.equal(p.batch["basecolor"], fit.fit_frames(g["base_color"], plan, "cpu"))
    assert p.batch["video"] is p.batch["depth"] and p.batch["depth"].dtype == BF and p.batch["env_ldr"].shape[2] == 17
    # fit off: the same clip reaches the pipeline as it is today (and would be refused by the tokenizer)
    node.run_forward_pass(p, g["depth"], g["normal"], g["roughness"], g["metallic"], g["base_color"], env, env_spin=90.0)
    assert p.batch["depth"].shape == (1, 3, 10, 40, 36) and p.batch["depth"].dtype == torch.float32
    assert torch.equal(p.batch["depth"], g["depth"].permute(0, 4, 1, 2, 3) * 2.0 - 1.0) and seen["env_spin"] == 90.0


def test_forward_node_refuses_gbuffers_of_different_sizes(pkg):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]()
    g = _gbuffers(3, 40, 36)
    g["roughness"] = R.source(1, 3, 40, 32)
    with pytest.raises(ValueError, match="'roughness'"):
        node.run_forward_pass(_Recorder(), g["depth"], g["normal"], g["roughness"], g["metallic"], g["base_color"],
                              torch.rand(1, 16, 32, 3), fit="stretch")


def test_inverse_node_fits_and_cuts(pkg):
    node = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]()
    p = _Recorder()
    image = R.source(1, 11, 70, 75)
    outs = node.run_inverse_pass(p, image, fit="crop")
    assert len(outs) == 5 and all(o.shape == (11, 64, 64, 3) for o in outs)
    fit = R.fit_module(pkg)
    assert torch.equal(p.batch["rgb"], fit.fit_frames(image, fit.plan_fit(11, 70, 75, "crop"), "cpu")) and p.batch["rgb"].shape[2] == 17
    # windows take any T: no padding when the clip will be windowed
    node.run_inverse_pass(p, R.source(1, 21, 70, 75), fit="crop", window_frames=9, window_overlap=2)
    assert p.batch["rgb"].shape == (1, 3, 21, 64, 64)
    node.run_inverse_pass(p, image, fit="off")
    assert torch.equal(p.batch["rgb"], image.permute(0, 4, 1, 2, 3) * 2.0 - 1.0)
