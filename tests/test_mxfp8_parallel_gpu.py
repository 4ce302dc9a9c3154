"""MXFP8 under sequence parallelism on real hardware: HipDiT(precision="mxfp8") and / or attention_precision="mxfp8" with a process
group.  As in tests/test_parallel_gpu.py the ranks share the one visible GPU and exchange over gloo (RCCL refuses two ranks on one
device); one case drives the real RCCL calls with a 1-rank group.  Weights and inputs are those of the bf16 sharded test.

Bit identity between a rank of the sharded run and the single-rank engine needs the same GEMM kernel and the same attention key
splits on both sides: the band (S / world rows) and the whole clip may fall on different sides of the few-token rule of the MXFP8
GEMM, so every worker switches that rule off for both engines (drn_gemm_mxfp8_force_small_m(0)), and asserts that the attention
plans of heads / world and of all heads cut the keys alike."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT, tiny_net

pytestmark = pytest.mark.gpu

_RDZV_N = [0]


def _rdzv():
    import tempfile
    _RDZV_N[0] += 1
    path = os.path.join(tempfile.gettempdir(), f"drn_mx_rdzv_{os.getpid()}_{_RDZV_N[0]}")
    if os.path.exists(path):
        os.remove(path)
    return "file://" + path


def _splits_by_row(plan):
    """An attention plan as merged (q0, q1, kv_splits) runs: what decides a query row's summation order."""
    out = []
    for q0, q1, ns in plan:
        if out and out[-1][2] == ns and out[-1][1] == q0:
            out[-1] = (out[-1][0], q1, ns)
        else:
            out.append((q0, q1, ns))
    return out


def _setup(pkg, wide, dev):
    net = tiny_net(pkg, 1024, 1, 8) if wide else tiny_net(pkg, 256, 2, 2)
    lat = (2, 64, 64) if wide else (2, 16, 16)
    if wide == "clip":
        lat = (8, 72, 128)                 # the headline clip's token count: a whole round + a split-KV tail, a two-part return
    sw = pkg.synthetic_weights
    sd = sw.synth_state_dict(net, torch.bfloat16, device=dev)
    x = sw.synth_tensor("pg.x", (1, 16) + lat, torch.float32, scale=2.0).to(torch.bfloat16).to(dev)
    cond = sw.synth_tensor("pg.c", (1, 16) + lat, torch.float32, scale=1.0).to(torch.bfloat16).to(dev)
    lib = pkg.native.load_library()
    if wide:
        lib.drn_gemm_force_tile(1)         # (the bf16 GEMMs that remain - patch embed, final layer - as in the bf16 test)
    lib.drn_gemm_mxfp8_force_small_m(0)
    return net, lat, sd, x, cond


class _Spy:
    """Counts the blocked MXFP8 GEMM launches and records the payload dtypes handed to the all-to-alls."""

    def __init__(self, pkg):
        self.blocked, self.payloads = 0, []
        Nn, eng = pkg.native, pkg.dit_engine
        real = Nn.gemm_mxfp8_blocked

        def blocked(*a, **k):
            self.blocked += 1
            return real(*a, **k)
        Nn.gemm_mxfp8_blocked = blocked
        for name in ("alltoall_rows_", "alltoall_bands_"):
            def wrap(send, *a, _real=getattr(eng, name), **k):
                self.payloads.append(tuple(t.dtype for t in send) if isinstance(send, (tuple, list)) else send.dtype)
                return _real(send, *a, **k)
            setattr(eng, name, wrap)

    def reset(self):
        self.blocked, self.payloads = 0, []

    def mx_returns(self):
        return [p for p in self.payloads if isinstance(p, tuple)]


MX_PAYLOAD = {torch.uint8, torch.float8_e4m3fn}


def _worker(rank, world, port, q, exchange, wide, mode):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["DRN_SP_EXCHANGE"] = exchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ.pop("DRN_SP_MX_RETURN", None)
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=world)
    try:
        from __graft_entry__ import load_package
        pkg = load_package()
        Nn, HipDiT = pkg.native, pkg.dit_engine.HipDiT
        dev = torch.device("cuda:0")
        net, lat, sd, x, cond = _setup(pkg, wide, dev)
        sw = pkg.synthetic_weights
        S, heads = lat[0] * lat[1] * lat[2] // 4, net["num_heads"]
        t, pg = torch.tensor(1.7), dist.group.WORLD
        spy = _Spy(pkg)
        res = {}
        if exchange == "a2a" and mode != "clip":
            assert _splits_by_row(Nn.attention_plan(1, heads // world, S, S)) == _splits_by_row(Nn.attention_plan(1, heads, S, S))

        def expect_path(eng, attention):
            p = eng.sp_path
            if exchange == "gather":
                assert p["layout"] == "gather", p
            else:
                # wide: the projections write / read the rank-major slabs through the blocked MXFP8 GEMM; tiny (128 columns per
                # rank): plain GEMM + regroup, and the bf16 return exchange (4-byte scale rows: the regroup cannot move them)
                slabs = bool(wide) and (eng._mx or net["model_channels"] // world >= 512)      # (bf16 slabs: from 512 columns)
                assert p["layout"] == ("slabs" if slabs else "regroup"), p
                if eng._mx:
                    assert (spy.blocked > 0) == bool(wide), spy.blocked
                    assert p["return"] == ("e4m3" if wide else "bf16"), p
            assert p["attention"] == attention, p

        if mode == "lin":
            single = HipDiT(net, sd, device=dev, precision="mxfp8")
            sharded = HipDiT(net, sd, device=dev, process_group=pg, precision="mxfp8")
            assert sharded.exchange == exchange
            y1 = single(x, t, cond, 2)
            y2 = sharded(x, t, cond, 2)
            torch.cuda.synchronize()
            expect_path(sharded, "bf16")
            res["sharded == single"] = bool(torch.equal(y1, y2))
            # two clips as ONE sharded batch against the same two clips one after the other
            xb = torch.cat([x, sw.synth_tensor("pg.x2", (1, 16) + lat, torch.float32, scale=2.0).to(torch.bfloat16).to(dev)], 0)
            cb = torch.cat([cond, sw.synth_tensor("pg.c2", (1, 16) + lat, torch.float32, scale=1.0).to(torch.bfloat16).to(dev)], 0)
            yb = sharded(xb, t, cb, [2, 4])
            y_one = torch.cat([sharded(xb[i:i + 1], t, cb[i:i + 1], ci) for i, ci in enumerate([2, 4])], 0)
            torch.cuda.synchronize()
            res["batch == clip by clip"] = (bool(torch.equal(yb, y_one)) and bool(torch.equal(yb[:1], y2))
                                            and not bool(torch.equal(yb[:1], yb[1:])))
        elif mode == "attn":
            Nn.attention_mxfp8_force(1)                          # the tiny clips are below the 2048-token rule
            for prec in ("bf16", "mxfp8"):
                spy.reset()
                single = HipDiT(net, sd, device=dev, precision=prec, attention_precision="mxfp8")
                sharded = HipDiT(net, sd, device=dev, process_group=pg, precision=prec, attention_precision="mxfp8")
                y1 = single(x, t, cond, 2)
                y2 = sharded(x, t, cond, 2)
                torch.cuda.synchronize()
                expect_path(sharded, "mxfp8")
                plain = HipDiT(net, sd, device=dev, precision=prec)(x, t, cond, 2)
                torch.cuda.synchronize()
                res[f"linears {prec}: sharded == single"] = bool(torch.equal(y1, y2))
                res[f"linears {prec}: the MXFP8 attention ran"] = not bool(torch.equal(y1, plain))
        elif mode == "switch":
            default = HipDiT(net, sd, device=dev, process_group=pg, precision="mxfp8")
            y_mx = default(x, t, cond, 2)
            torch.cuda.synchronize()
            assert default.sp_path["return"] == "e4m3", default.sp_path
            sent = spy.mx_returns()
            assert sent and all(set(p) <= MX_PAYLOAD and len(p) == 2 for p in sent), spy.payloads
            spy.reset()
            os.environ["DRN_SP_MX_RETURN"] = "0"
            bf = HipDiT(net, sd, device=dev, process_group=pg, precision="mxfp8")
            os.environ.pop("DRN_SP_MX_RETURN")
            y_bf = bf(x, t, cond, 2)
            torch.cuda.synchronize()
            assert bf.sp_path["return"] == "bf16" and not spy.mx_returns() and spy.blocked > 0, (bf.sp_path, spy.payloads)
            res["e4m3 return == bf16 return + quantise launch"] = bool(torch.equal(y_mx, y_bf))
        elif mode == "clip":
            ap = Nn.attention_plan(1, heads // world, S, S)
            sharded = HipDiT(net, sd, device=dev, process_group=pg, precision="mxfp8")
            assert len(ap) == 2 and ap[0][1] // (S // world) >= 1 and sharded._split_return
            y2 = sharded(x, t, cond, 2)
            torch.cuda.synchronize()
            expect_path(sharded, "bf16")
            assert len(spy.mx_returns()) == 2 * net["num_blocks"], spy.payloads          # the two parts of every layer's return
            whole = HipDiT(net, sd, device=dev, process_group=pg, precision="mxfp8")
            whole._split_return = False
            y3 = whole(x, t, cond, 2)
            torch.cuda.synchronize()
            res["two-part return == one collective"] = bool(torch.equal(y2, y3))
            y_bf = HipDiT(net, sd, device=dev)(x, t, cond, 2).float()
            y_mx = HipDiT(net, sd, device=dev, precision="mxfp8")(x, t, cond, 2).float()
            torch.cuda.synchronize()
            res["d_single"] = float((y_mx - y_bf).norm() / y_bf.norm())
            res["d_sharded"] = float((y2.float() - y_bf).norm() / y_bf.norm())
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def _spawn(world, exchange, wide, mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _rdzv()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, exchange, wide, mode)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    return sorted(q.get(timeout=10) for _ in range(world))


CASES = [("a2a", False, 2), ("gather", False, 2), ("a2a", True, 2), ("a2a", True, 4)]


@pytest.mark.parametrize("exchange,wide,world", CASES)
def test_sharded_mxfp8_equals_single_rank(gpu, exchange, wide, world):
    """precision="mxfp8" with a process group: the sharded output is the single-rank mxfp8 output, bit for bit - blocked MXFP8 GEMM
    and e4m3 return exchange (wide), plain GEMM + regroup (tiny), K|V gather - and a sharded batch equals its clips one by one."""
    for rank, res in _spawn(world, exchange, wide, "lin"):
        print(f"rank {rank}: {res}")
        assert all(res.values()) and len(res) == 2, f"rank {rank}: {res}"


@pytest.mark.parametrize("exchange,wide,world", CASES)
def test_sharded_mxfp8_attention_equals_single_rank(gpu, exchange, wide, world):
    """attention_precision="mxfp8" with a process group (forced on: the clips are below the 2048-token rule), once with bf16 and
    once with mxfp8 block linears: bit for bit the single-rank engine of the same two precisions."""
    for rank, res in _spawn(world, exchange, wide, "attn"):
        print(f"rank {rank}: {res}")
        assert all(res.values()) and len(res) == 4, f"rank {rank}: {res}"


def test_return_exchange_switch(gpu):
    """DRN_SP_MX_RETURN=0 (bf16 return exchange + a quantise launch) against the default (the attention epilogue's e4m3 elements and
    scales travel, as uint8 / fp8 payloads): the same bits."""
    for rank, res in _spawn(2, "a2a", True, "switch"):
        assert all(res.values()) and len(res) == 1, f"rank {rank}: {res}"


def test_headline_clip_geometry(gpu):
    """18 432 tokens on 2 ranks, mxfp8 linears, e4m3 return in two parts.  A rank's split-KV tail differs from the single-rank
    one here, so only the exchange can be bit-exact: two-part return == one collective.  Against the single rank the yardstick is
    the quantisation error itself: rel-L2 to the single-rank bf16 output of the sharded mxfp8 run within 1.1 x that of the
    single-rank mxfp8 run (a different fp32 summation order in the split-KV combine is a bf16-ulp effect, rel < 2e-3 in the bf16
    case; the MXFP8 error is several times that)."""
    for rank, res in _spawn(2, "a2a", "clip", "clip"):
        print(f"rank {rank}: d_single={res['d_single']:.4e} d_sharded={res['d_sharded']:.4e} "
              f"ratio={res['d_sharded'] / res['d_single']:.4f}")
        assert res["two-part return == one collective"], f"rank {rank}"
        assert res["d_sharded"] <= 1.1 * res["d_single"], (res["d_sharded"], res["d_single"])


def _rccl_worker(port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["DRN_SP_EXCHANGE"] = "a2a"
    os.environ.pop("DRN_SP_MX_RETURN", None)
    import torch.distributed as dist
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=port, rank=0, world_size=1, device_id=dev)
    try:
        from __graft_entry__ import load_package
        pkg = load_package()
        pkg.parallel.SINGLE_RANK_COLLECTIVES = True
        net, lat, sd, x, cond = _setup(pkg, False, dev)
        spy = _Spy(pkg)
        y1 = pkg.dit_engine.HipDiT(net, sd, device=dev, precision="mxfp8")(x, torch.tensor(1.7), cond, 2)
        eng = pkg.dit_engine.HipDiT(net, sd, device=dev, process_group=dist.group.WORLD, precision="mxfp8")
        assert eng.exchange == "a2a"
        for _ in range(3):                                       # repeated: buffer reuse across async exchanges
            y2 = eng(x, torch.tensor(1.7), cond, 2)
        torch.cuda.synchronize()
        sent = spy.mx_returns()
        q.put({"same": bool(torch.equal(y1, y2)), "return": eng.sp_path["return"],
               "payloads ok": bool(sent) and all(set(p) <= MX_PAYLOAD for p in sent)})
    finally:
        dist.destroy_process_group()


def test_e4m3_return_over_rccl_single_rank(gpu):
    """The real transport: a 1-rank RCCL group carries the e4m3 elements and the scale bytes of the return exchange
    (all_to_all_single on uint8 views of device buffers) and must not change a bit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_rdzv(), q))
    p.start()
    p.join(timeout=300)
    assert p.exitcode == 0
    res = q.get(timeout=10)
    assert res == {"same": True, "return": "e4m3", "payloads ok": True}, res
