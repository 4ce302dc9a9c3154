"""Cosmos1Relight on the CPU, with recorder pipelines that honour `to_host`: what the forward stage is handed, the six outputs
against the inverse node followed by the forward node, the composition by hand with fit_restore, the refusal of a cutting crop
before anything runs, and the registration rule."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

import fit_refs as R
from conftest import ROOT

BF = torch.bfloat16
GBUFFERS = ("basecolor", "metallic", "roughness", "normal", "depth")          # the inverse node's order


class _Pipe:
    """Stands where the pipeline stands, for both renderers: answers with bytes computed from the batch it is handed (so a
    different batch is a different answer), applies a restore plan as the pipeline does, honours `to_host`, and keeps what it saw."""
    device = "cpu"

    def __init__(self, fit, batch_passes=False):
        self.fit, self.batch_passes, self.restore_plan = fit, batch_passes, None
        self.calls, self.forward_batch, self.inverse_outs, self.ways = 0, None, [], []

    def set_model_type(self, t):
        self.model_type = t

    def _frames(self, batch, k):
        if self.model_type == "inverse":
            x = (batch["video"].float() + 1.0) * 100.0 + 9.0 * k
        else:
            self.forward_batch = dict(batch)
            x = sum(batch[n].float() * (i + 1) for i, n in enumerate(GBUFFERS))
            x = (x + 15.0) * 8.0 + 40.0 * batch["env_ldr"].float().mean(dim=(1, 3, 4))[:, None, :, None, None]
        u8 = x.permute(0, 2, 3, 4, 1).round().clamp(0, 255).to(torch.uint8).contiguous()
        if self.model_type == "inverse":
            self.inverse_outs.append(u8)
        if self.restore_plan is not None:
            u8 = self.fit.restore_frames(u8, dataclasses.replace(self.restore_plan, T=min(u8.shape[1], self.restore_plan.T)))
        return u8

    def _render(self, way, batch, k, to_host):
        self.calls += 1
        self.ways.append(way)
        u8 = self._frames(batch, k)
        return u8.numpy() if to_host else u8

    def generate_video(self, data_batch, normalize_normal=False, seed=None, to_host=True):
        k = int(data_batch["context_index"][0, 0]) if "context_index" in data_batch else 0
        return self._render("one", data_batch, k, to_host)

    def generate_video_each(self, data_batches, normalize_normal, seed=None, to_host=True):
        return [self._render("each", b, int(b["context_index"][0, 0]), to_host) for b in data_batches]

    def generate_video_passes(self, data_batch, normalize_normal, seed=None, to_host=True):
        return [self._render("passes", data_batch, int(k), to_host) for k in data_batch["context_index"][:, 0]]


@pytest.fixture(scope="module")
def fit(pkg):
    return R.fit_module(pkg)


@pytest.fixture(scope="module")
def env():
    return torch.rand(1, 16, 32, 3, generator=torch.Generator().manual_seed(5)) * 3.0


def _relight(pkg):
    return pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]()


def _chain(pkg, p, image, env, inv_kw, fwd_kw):
    """The two nodes joined through the host: the inverse node's G-buffers, 5-D again, into the forward node."""
    g = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(p, image, seed=3, **inv_kw)
    B = image.shape[0]
    g5 = dict(zip(("base_color", "metallic", "roughness", "normal", "depth"), (o.reshape(B, -1, *o.shape[1:]) for o in g)))
    (relit,) = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"]().run_forward_pass(
        p, g5["depth"], g5["normal"], g5["roughness"], g5["metallic"], g5["base_color"], env, seed=3, **fwd_kw)
    return (relit, *g)


CASES = {
    "fit_off": ((9, 64, 64), dict()),
    "crop_time_padding": ((11, 70, 75), dict(fit="crop")),
    "windows": ((21, 70, 75), dict(fit="crop", window_frames=9, window_overlap=2)),
}


@pytest.mark.parametrize("batch_passes", (False, True), ids=("pass_by_pass", "batched_passes"))
@pytest.mark.parametrize("name", list(CASES))
def test_relight_equals_the_two_node_chain(pkg, fit, env, name, batch_passes):
    (T, H, W), kw = CASES[name]
    image = R.source(1, T, H, W, seed=11)
    win = {k: v for k, v in kw.items() if k.startswith("window")}
    light = dict(env_spin=90.0, env_rotation=180.0, env_brightness=1.5)
    p = _Pipe(fit, batch_passes)
    got = _relight(pkg).run_relight(p, p, image, env, seed=3, **light, **kw)
    ways = list(p.ways)
    assert ways[:-1] == {False: ["each"] * 5 if win else ["one"] * 5, True: ["passes"] * 5}[batch_passes] and ways[-1] == "one"
    # what the forward stage was handed: the uint8 G-buffers through fit_frames under the forward node's own plan
    Hm, Wm = H // 16 * 16, W // 16 * 16
    plan = fit.plan_fit(T, Hm, Wm, "crop", 0, 0, windowed=bool(win) and T > win["window_frames"])
    assert len(p.inverse_outs) == 5 and p.inverse_outs[0].shape[2:4] == (Hm, Wm)
    for n, u8 in zip(GBUFFERS, p.inverse_outs):
        assert u8.dtype == torch.uint8 and p.forward_batch[n].dtype == BF
        assert torch.equal(p.forward_batch[n], fit.fit_frames(u8[:, :T], plan, "cpu")), n
    assert p.forward_batch["video"] is p.forward_batch["depth"] and p.forward_batch["depth"].shape[2] == plan.T_out
    # the six outputs
    q = _Pipe(fit, batch_passes)
    want = _chain(pkg, q, image, env, kw, dict(light, fit="crop", **win))
    assert len(got) == 6 and got[0].shape == (1, T, Hm, Wm, 3) and all(o.shape == (T, Hm, Wm, 3) for o in got[1:])
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    assert not torch.equal(got[1], got[2]) and float(got[0].std()) > 0
    assert p.restore_plan is None


def test_relight_with_fit_restore_is_the_composition_by_hand(pkg, fit, env):
    T, H, W = 10, 40, 36
    image = R.source(1, T, H, W, seed=12)
    p = _Pipe(fit)
    got = _relight(pkg).run_relight(p, p, image, env, seed=3, env_spin=45.0, fit="stretch", fit_restore=True)
    assert got[0].shape == (1, T, H, W, 3) and all(o.shape == (T, H, W, 3) for o in got[1:])
    rplan = fit.plan_restore(fit.plan_fit(T, H, W, "stretch"))
    q = _Pipe(fit)
    small = _chain(pkg, q, image, env, dict(fit="stretch"), dict(env_spin=45.0, fit="crop"))      # everything at the model's size
    assert small[0].shape == (1, T, 32, 32, 3)
    for a, s in zip(got, small):
        u8 = (s * 255.0).round().to(torch.uint8).reshape(1, T, 32, 32, 3)
        assert torch.equal(u8.float() / 255.0, s.reshape(1, T, 32, 32, 3))
        assert torch.equal(a.reshape(1, T, H, W, 3), fit.restore_frames(u8, rplan).float() / 255.0)
    # the G-buffers are also what the inverse node returns with fit_restore
    inv = pkg.NODE_CLASS_MAPPINGS["Cosmos1InverseRenderer"]().run_inverse_pass(q, image, seed=3, fit="stretch", fit_restore=True)
    assert all(torch.equal(a, b) for a, b in zip(got[1:], inv))


def test_a_cutting_crop_with_restore_is_refused_before_anything_runs(pkg, fit, env):
    a, b = _Pipe(fit), _Pipe(fit)
    with pytest.raises(ValueError, match="crop cannot be undone"):
        _relight(pkg).run_relight(a, b, R.source(1, 10, 40, 36), env, fit="crop", fit_restore=True)
    assert a.calls == 0 and b.calls == 0
    out = _relight(pkg).run_relight(a, b, R.source(1, 10, 40, 36), env, fit="crop")             # two pipeline objects
    assert a.calls == 5 and b.calls == 1 and out[0].shape == (1, 10, 32, 32, 3)


def test_relight_declares_its_surface(pkg):
    cls = pkg.nodes.EXTRA_NODE_CLASS_MAPPINGS["Cosmos1Relight"]
    assert cls.FUNCTION == "run_relight" and cls.CATEGORY == "Cosmos1" and cls.RETURN_TYPES == ("IMAGE",) * 6
    assert cls.RETURN_NAMES == ("image", "base_color", "metallic", "roughness", "normal", "depth")
    types = cls.INPUT_TYPES()
    assert list(types["required"]) == ["inverse_pipeline", "forward_pipeline", "image", "env_map"]
    fwd = pkg.NODE_CLASS_MAPPINGS["Cosmos1ForwardRenderer"].INPUT_TYPES()["optional"]
    for k in ("guidance", "forward_guidance", "seed", "env_format", "env_brightness", "env_flip_horizontal", "env_rotation",
              "env_spin", "window_frames", "window_overlap", "fit", "fit_height", "fit_width", "fit_restore"):
        assert k in types["optional"], k
        if k.startswith("env_"):
            assert types["optional"][k] == fwd[k]
    assert pkg.nodes.EXTRA_NODE_DISPLAY_NAME_MAPPINGS == {"Cosmos1Relight": "Cosmos1 Relight"}


def test_extra_nodes_are_exported_only_on_request(pkg):
    assert len(pkg.NODE_CLASS_MAPPINGS) == 4 and "Cosmos1Relight" not in pkg.NODE_CLASS_MAPPINGS
    assert len(pkg.NODE_DISPLAY_NAME_MAPPINGS) == 4
    code = ("from __graft_entry__ import load_package; p = load_package(); "
            "print(len(p.NODE_CLASS_MAPPINGS), len(p.NODE_DISPLAY_NAME_MAPPINGS), 'Cosmos1Relight' in p.NODE_CLASS_MAPPINGS)")
    base = {k: v for k, v in os.environ.items() if k != "DRN_EXTRA_NODES"}
    base["HIP_VISIBLE_DEVICES"] = ""            # the child stays on the CPU
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(base, DRN_EXTRA_NODES="1"), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "5 5 True", out.stdout
