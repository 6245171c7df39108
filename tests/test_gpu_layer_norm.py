"""Runtime.layer_norm on the GPU (csrc/fc_layernorm.hip).  Tolerance of the kernel tests: the error of an fp32 evaluation
on the CPU (torch's layer_norm; the backward: the fp32 oracle in the kernel's chunk order) against the same fp64
reference on the same inputs is measured here and four times that is allowed (another summation order); bf16 planes
add their representation error, 2^-17 relative for a hi + lo pair and 2^-8 for one bf16 plane."""
import numpy as np
import pytest
import torch
from head_fixtures import fill_replay

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 1e-5
KINDS = {"scalar": {}, "c51": {"num_atoms": 3}, "implicit": {"num_atoms": 8, "dist_head": "implicit"},
         "munchausen": {"munchausen": True}, "noisy": {"noisy": True}}


def _split(v, split):
    hi = v.to(torch.bfloat16)
    return hi, ((v - hi.float()).to(torch.bfloat16) if split else None)


def _join64(hi, lo):
    return hi.double().cpu() if lo is None else hi.double().cpu() + lo.double().cpu()


def _err(a, b):
    return (a.double().cpu() - b).abs()


def _fc_ln(M, switch, save_n, ksplit, split, zero_first=False):
    """fc_fwd(ln=): the kernel's (h, xhat, rstd), fp64 pre-activations from the GEMM's own partial planes, gamma, beta."""
    from apex_dqn_amd.ops import conv as C
    from apex_dqn_amd.ops.fused_ops import HipBackend
    ops = HipBackend()
    g = torch.Generator().manual_seed(M * 7 + ksplit)
    rnd = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(DEV)          # noqa: E731
    x, x_lo = _split(rnd(M, 3136).relu(), split)
    w, w_lo = _split(rnd(1024, 3136, k=0.0 if zero_first else 0.03), split)
    w2, w2_lo = _split(rnd(1024, 3136, k=0.03), split)
    b, b2 = (torch.full((1024,), 0.37, device=DEV) if zero_first else rnd(1024)), rnd(1024)
    gam = [torch.rand(1024, generator=g).to(DEV) + 0.5 for _ in range(2)]
    bet = [(torch.randint(-8, 9, (1024,), generator=g) / 8).to(DEV) for _ in range(2)]      # exact in one bf16 plane
    out, out_lo = _split(torch.zeros(M, 1024, device=DEV), split)
    lo = dict(x_lo=x_lo, w_lo=w_lo, w2_lo=w2_lo, out_lo=out_lo) if split else {}
    part, nz = C.dense_fwd128(ops.lib, ops.ws, x, w, b, out, True, w2, b2, switch, ksplit, True, no_epilogue=True, **lo)
    rows2 = (torch.arange(M) >= switch)[:, None]
    a64 = part[:nz * M * 1024].double().reshape(nz, M, 1024).sum(0).cpu() + torch.where(rows2, b2.cpu(), b.cpu()).double()
    xhat, rstd = torch.full((save_n + 2, 1024), -7.0, device=DEV), torch.full((save_n + 2, 2), -7.0, device=DEV)
    ops.fc_fwd(x, w, b, out, w2, b2, switch, ksplit=ksplit, ln=(gam[0], bet[0], gam[1], bet[1], EPS, save_n, xhat, rstd), **lo)
    return (_join64(out, out_lo), xhat.cpu(), rstd.cpu(), a64, torch.where(rows2, gam[1].cpu(), gam[0].cpu()),
            torch.where(rows2, bet[1].cpu(), bet[0].cpu()))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize("save_n", [0, 2])
@pytest.mark.parametrize("M,switch,const", [(3, 2, False), (130, 87, False), (3, 2, True)])
def test_epilogue_kernel(M, switch, const, save_n, ksplit, split):
    """``const``: zero weights and a constant bias in the first set, rows of identical pre-activations."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    h, xhat, rstd, a64, gm, bt = _fc_ln(M, switch, save_n, ksplit, split, const)
    h_ref, xh_ref, r_ref = TorchBackend.fc_ln_fwd(a64, gm.double(), bt.double(), EPS)
    xh32, _, r32 = torch.native_layer_norm(a64.float().reshape(M, 2, 512), (512,), None, None, EPS)      # the stand-in
    e_x, e_r = float(_err(xh32.reshape(M, 1024), xh_ref).max()), float(_err(r32.reshape(M, 2), r_ref).max())
    e_h = float(_err(torch.relu(gm * xh32.reshape(M, 1024) + bt), h_ref).max())
    assert bool((_err(h, h_ref) <= 4 * e_h + (2.0 ** -17 if split else 2.0 ** -8) * h_ref.abs()).all())
    assert bool((_err(xhat[:save_n], xh_ref[:save_n]) <= 4 * e_x).all() and (_err(rstd[:save_n], r_ref[:save_n]) <= 4 * e_r).all())
    assert bool((xhat[save_n:] == -7.0).all()) and bool((rstd[save_n:] == -7.0).all())      # canaries
    if const:       # xh = 0 and h = max(beta, 0) exactly, no NaN
        assert bool((a64[:2] == a64[0, 0]).all()) and bool((xhat[:save_n] == 0).all()) and not bool(torch.isnan(h).any())
        assert torch.equal(h[:2], bt[:2].double().clamp_min(0))
        assert bool((rstd[:save_n] == np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))).all())


@pytest.mark.parametrize("name,feat,off", [("features", 1000, 0), ("xhat", 1024, 4), ("save_n", 1024, 0)])
def test_launchers_refuse_naming_the_argument(name, feat, off):
    """A feature count that is not 2 x 512, a pointer off 16-byte alignment, save_n above M."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    ops, z = HipBackend(), (lambda *s: torch.zeros(*s, device=DEV))
    with pytest.raises(ValueError, match=name):
        _ = name == "save_n" and _fc_ln(3, 2, 9, 1, False)
        a = ops.fc_ln_args(z(4, 1024).bfloat16(), z(4, 1024), z(4, 2), z(1024), z(1024), z(1024))
        a.features, a.xhat = feat, a.xhat + off
        ops.fc_ln_reduce(a)


def _chunk_order_fp32(dz, xh, chunk):
    """G[gamma], G[beta] in fp32 in the kernel's order: a wave's rows w, w + 4, ..., then the waves, then the chunks."""
    t, tot = torch.stack([dz * xh, dz], 1), 0
    for c0 in range(0, len(dz), chunk):
        tot = tot + sum(sum(t[m] for m in range(c0 + w, min(c0 + chunk, len(dz)), 4)) for w in range(4))
    return tot


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("chunks,extra", [(0, 1), (0, 5), (3, 1)])
def test_backward_kernel(chunks, extra, split):
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend
    ops = HipBackend()
    chunk = int(ops.lib.apex_fc_ln_chunk())
    B = chunks * chunk + extra          # 1, 5 (below one chunk, four does not divide it), 3 chunks + 1
    g = torch.Generator().manual_seed(B)
    gamma = torch.rand(1024, generator=g) + 0.5
    a = torch.randn(B, 1024, generator=g, dtype=torch.float64) * 2 + 0.5
    xh, r = (t.float() for t in TorchBackend.fc_ln_fwd(a, gamma.double(), torch.zeros(1024).double(), EPS)[1:])
    dz = torch.randn(B, 1024, generator=g) * (torch.rand(B, 1024, generator=g) < 0.5)
    dz[B - 1] *= float(B == 1)          # one all-zero row (kept when it is the only row)
    hi, lo = _split(dz.to(DEV), split)
    dz64 = _join64(hi, lo)              # the fp32 value of the planes
    # fp64 autograd of the definition at a = xh / r with, per (row, stream), the eps that makes 1 / sqrt(var + eps) = r
    a64 = (xh.double().reshape(B, 2, 512) / r.double()[..., None]).requires_grad_(True)
    g64, b64 = gamma.double().reshape(2, 512).clone().requires_grad_(True), torch.zeros(2, 512).double().requires_grad_(True)
    d = a64 - a64.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    z = g64 * (d / torch.sqrt(var + (1.0 / r.double()[..., None] ** 2 - var).detach())) + b64
    (z * dz64.reshape(B, 2, 512)).sum().backward()
    ref = (a64.grad.reshape(B, 1024), g64.grad.reshape(1024), b64.grad.reshape(1024))
    std = (TorchBackend.fc_ln_bwd(dz64.float(), xh, r, gamma)[0], *_chunk_order_fp32(dz64.float(), xh, chunk))
    e = [float(_err(s, q).max()) for s, q in zip(std, ref)]

    def run():
        h, l = hi.clone(), (lo.clone() if split else None)
        gg, gb = torch.full((1024,), 9.0, device=DEV), torch.full((1024,), 9.0, device=DEV)
        ops.fc_ln_reduce(ops.fc_ln_backward(h, xh.to(DEV), r.to(DEV), gamma.to(DEV), gg, gb, dh_lo=l))
        return h, l, gg, gb

    h, l, gg, gb = run()
    dd = [_err(_join64(h, l), ref[0]), _err(gg, ref[1]), _err(gb, ref[2])]
    assert bool((dd[0] <= 4 * e[0] + (2.0 ** -17 if split else 2.0 ** -8) * ref[0].abs()).all())
    assert bool((dd[1] <= 4 * e[1]).all()) and bool((dd[2] <= 4 * e[2]).all())
    assert all(x is None or torch.equal(x, y) for x, y in zip((h, l, gg, gb), run()))      # a second launch: the same bits


def _learner(kind, dtype, backend="hip", split=None, **rt):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                "Actor": {"num_actors": 24}, "Learner": {"replay_sample_size": 64, "q_target_sync_freq": 1000},
                                "Runtime": {"layer_norm": True, "dtype": dtype, **KINDS[kind], **rt}})
    torch.manual_seed(0)
    rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
    fill_replay(rp, 1500, seed=11)
    L = FusedNatureLearner(cfg, DEV, rp, backend=backend, split=split)
    g = torch.Generator().manual_seed(5)
    for V in (L.P, L.T):        # gamma / beta off their start, the two nets apart
        V["lng"].copy_(torch.rand(1024, generator=g) + 0.5)
        V["lnb"].copy_(torch.randn(1024, generator=g) * 0.2)
    L._refresh_bf16()
    L._target_changed()
    return L


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_learner_step_and_graphs(kind, dtype):
    """Every gradient segment of one update within tests/test_gpu_split.py's 1e-3 (norm-wise) of the torch backend's in
    fp32; the bf16-operand step (there bounded only against the split step): the sibling whole-step tests' 0.2.  Then
    three replays of the one-update graph and one of the three-update graph == six eager updates, bit for bit."""
    res = {}
    for be in ("hip", "torch"):
        L = _learner(kind, dtype, be, split=dtype == "fp32", use_graphs=False, presample=False)
        assert L.layer_norm and not L._fuse_norm and not L._defer_fc_epilogue
        L.ops.dtype = torch.float32 if be == "torch" else L.ops.dtype
        L._step_body()
        res[be] = dict(L.layout.views(L.g32.clone()), td_abs=L.td_abs.clone(), idx=L.S["idx"].float(), rstd=L.ln_rstd.clone())
    errs = {k: float((v - res["torch"][k]).norm() / (res["torch"][k].norm() + 1e-12)) for k, v in res["hip"].items()}
    assert max(errs.values()) < (1e-3 if dtype == "fp32" else 0.2), errs
    assert errs["idx"] == 0 and float(res["hip"]["lng"].norm()) > 0 and float(res["hip"]["lnb"].norm()) > 0
    for graphs in (True, False):
        L = _learner(kind, dtype, use_graphs=graphs, graph_steps=3, target_ema_rate=0.01)
        for _ in range(3):
            L.step()
        L.steps(3)
        assert (L._graphs is not None) == graphs == (L._multi is not None) and L.num_q_updates == 6
        res[graphs] = [t.clone() for t in (L.p32, L._pbf_all, L.rms_v, L.rms_m, L.t32, L._tbf_all)]
        assert not torch.equal(res[graphs][0][L.layout.offsets["lng"]:], res[graphs][4][L.layout.offsets["lng"]:])     # it trails
    assert all(torch.equal(a, b) for a, b in zip(res[True], res[False]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_actor_group_and_reset(dtype):
    from apex_dqn_amd.actors.gpu_actor import GpuActorGroup
    from apex_dqn_amd.envs.vector_envs import make_vec_env
    from apex_dqn_amd.models.dueling import DuellingDQN
    from apex_dqn_amd.models.flat_params import flat_to_reference_state
    L = _learner("scalar", dtype, use_graphs=False, reset_interval=50, reset_shrink_head=0.0)
    E, A, rp, cfg = 24, 6, L.replay, L.cfg
    grp = GpuActorGroup(cfg, L, rp, make_vec_env(cfg.env_backend, cfg.env_conf.name, E, A, seed=0), E)
    seqs = rp.append_frames(np.random.default_rng(5).integers(0, 255, (E + 8, 84, 84), dtype=np.uint8))
    payload = np.stack([seqs[i:i + 4] for i in range(E)])
    frames = rp.gather_frames(torch.from_numpy((payload % rp.F).astype(np.int32)).to(DEV))
    net = DuellingDQN((4, 84, 84), A, obs_scale=cfg.Runtime.obs_scale, **cfg.head_kw()).to(DEV)
    net.load_state_dict(flat_to_reference_state(grp.P, 64))
    q_ref = net(frames)[2].detach().double().cpu()
    grp.eps.zero_()
    err = float(_err(torch.from_numpy(grp.policy(payload)[0]), q_ref).max())
    # tests/test_gpu_noisy.py's actor bound (split kernels); bf16: the 5e-2 its whole-step test allows td_abs, a q-derived value
    assert err < (1e-4 if dtype == "fp32" else 5e-2), err
    L.reset_now(1)
    assert all(bool((V["lng"] == 1).all()) and bool((V["lnb"] == 0).all()) for V in (L.P, L.T))
