"""Factorised NoisyNet fc and head layers on the GPU: csrc/noisy.hip against the host mirror
(learner/noisy.py) and the torch-backend oracle, the whole step against the torch backend,
graph capture with the draw index read on the device, the actor group, the GPU loop and
resume."""
import functools

import numpy as np
import pytest
import torch
from head_fixtures import fill_replay

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(2, 1), (3, 7), (18, 64)]     # head rows 1 / 2, 7 / 21 (no multiple of a row tile), 64 / 1152


# --------------------------------------------------------------------- harness
def _ulp32(ref64):
    """Spacing of fp32 at |ref| (fp64 tensor)."""
    r = ref64.float().abs()
    return (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()


def _gauss(xi):
    """g = sign(xi) xi^2 of a draw (fp64)."""
    x = xi.double()
    return torch.sign(x) * x * x


@functools.lru_cache(maxsize=None)
def _params(A, N, zero_sigma=False):
    """Flat parameters (CPU) of two nets in the noisy layout: mu ~ U(-0.05, 0.05), sigma ~
    U(0, 0.02) -- the scale at which mu and the noise term cancel to small values often."""
    from apex_dqn_amd.models.flat_params import FlatLayout, nature_segments
    lay = FlatLayout(nature_segments(4, A, 64, N, noisy=True))
    mu = FlatLayout(nature_segments(4, A, 64, N))
    g = torch.Generator().manual_seed(11)
    p = (torch.rand(2, lay.numel, generator=g) - 0.5) * 0.1
    for s in ("swv", "sbv", "swa", "sba", "swfc", "sbfc"):
        o = lay.offsets[s]
        n = int(np.prod(lay.shapes[s]))
        p[:, o:o + n] = 0.0 if zero_sigma else torch.rand(2, n, generator=g) * 0.02
    return lay, mu, p


def _plan(lay, A, N, u, every=1, stream0=0, base=1000):
    from apex_dqn_amd.learner.noisy import NoisyPlan, noise_seed
    ctr = torch.tensor([base + u], dtype=torch.int64, device=DEV)
    b = torch.tensor([base], dtype=torch.int64, device=DEV)
    return NoisyPlan(A=A, N=N, offsets=dict(lay.offsets), seed=noise_seed(3), ctr=ctr, base=b, every=every,
                     stream0=stream0)


def _compose(A, N, split, u, zero_sigma=False, nnets=2, fc32=True):
    """One ``noisy_compose`` launch on sentinel-filled shadows; everything back as a dict."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    lay, mu, p = _params(A, N, zero_sigma)
    plan = _plan(lay, A, N, u)
    nm = mu.numel
    pd = p.to(DEV)
    e32 = torch.full((nnets, nm), 7.0, device=DEV)
    ebf = torch.full((nnets, (2 if split else 1) * nm), 3.0, device=DEV, dtype=torch.bfloat16)
    xi = torch.full((nnets, (plan.K + 63) // 64 * 64), -9.0, device=DEV)
    f32 = [torch.full((1024, 3136), 5.0, device=DEV) for _ in range(nnets)] if fc32 else None
    nets = [(pd[i], e32[i], ebf[i, :nm], ebf[i, nm:] if split else None) for i in range(nnets)]
    HipBackend().noisy_compose(plan, nets, xi, fc32=f32)
    torch.cuda.synchronize()
    return dict(lay=lay, mu=mu, plan=plan, p=pd, e32=e32, ebf=ebf, xi=xi, fc32=f32, nm=nm, nets=nets)


# ------------------------------------------------------- 1. xi vs the host mirror
@pytest.mark.parametrize("A,N", SHAPES)
def test_device_xi_vs_mirror(A, N):
    """Both nets, two update indices.  Tolerance 2e-5 absolute on the Gaussian draws g = sign(xi)
    xi^2: the fp32 argument of the cosine carries <= 2 pi 2^-24 = 3.7e-7, times a radius <=
    sqrt(2 ln 2^24) = 5.8 gives 2.2e-6; a few ulp of logf / sqrtf / cospif at magnitude <= 5.8 add
    about 2e-6; the bound is about 4x that sum."""
    from apex_dqn_amd.learner.noisy import gaussians
    worst = 0.0
    for u in (0, 123457):
        r = _compose(A, N, False, u, fc32=False)
        K = r["plan"].K
        assert K == 2 * 3136 + 1024 + 2 * 512 + N + A * N
        for net in (0, 1):
            g_ref = torch.from_numpy(gaussians(r["plan"].seed, u, net, K))
            err = float((_gauss(r["xi"][net, :K].cpu()) - g_ref).abs().max())
            worst = max(worst, err)
            assert bool((r["xi"][net, K:] == -9.0).all())             # nothing past the draw
        assert not torch.equal(r["xi"][0, :K], r["xi"][1, :K])
    print(f"(A, N) = ({A}, {N}): max |g_device - g_mirror| = {worst:.3e}")
    assert worst <= 2e-5, worst


def test_draw_index_divides_by_the_resample_period():
    """u = (ctr - base) // every, stream = stream0 + net: an actor group's plan (one net)."""
    from apex_dqn_amd.learner.noisy import gaussians
    from apex_dqn_amd.ops.fused_ops import HipBackend
    A, N = 3, 7
    lay, mu, p = _params(A, N)
    pd = p.to(DEV)
    nm = mu.numel
    got = []
    for calls in (6, 8, 9):
        plan = _plan(lay, A, N, calls, every=3, stream0=5, base=0)
        plan.base = None
        xi = torch.zeros(1, (plan.K + 63) // 64 * 64, device=DEV)
        HipBackend().noisy_compose(plan, [(pd[0], torch.zeros(nm, device=DEV),
                                           torch.zeros(nm, device=DEV, dtype=torch.bfloat16), None)], xi)
        torch.cuda.synchronize()
        got.append(xi[0, :plan.K].cpu())
        g_ref = torch.from_numpy(gaussians(plan.seed, calls // 3, 5, plan.K))
        assert float((_gauss(got[-1]) - g_ref).abs().max()) <= 2e-5
    assert torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


# ------------------------------------------------- 2. compose vs the fp64 value
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("A,N", SHAPES)
def test_noisy_compose_vs_oracle(A, N, split):
    """Effective fp32 values within 1 fp32 ulp of mu + sigma (xi_out xi_in) evaluated in fp64 from
    the device's own draw (the ulp covers FMA contraction and double rounding), and of the
    torch-backend oracle fed that draw; planes bit-equal to the project's split / bf16 rounding
    of the fp32 value the kernel reported; shadow regions outside the six segments untouched."""
    from apex_dqn_amd.learner import noisy as NZ
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    r = _compose(A, N, split, 17)
    plan, nm, lay = r["plan"], r["nm"], r["lay"]
    K = plan.K
    # the oracle on the device's draws
    o32 = torch.full_like(r["e32"], 7.0)
    obf = torch.full_like(r["ebf"], 3.0)
    of32 = [torch.zeros(1024, 3136, device=DEV) for _ in range(2)]
    oxi = torch.zeros_like(r["xi"])
    TorchBackend().noisy_compose(plan, [(r["p"][i], o32[i], obf[i, :nm], obf[i, nm:] if split else None)
                                        for i in range(2)], oxi, fc32=of32, xi_in=r["xi"])
    worst = 0.0
    touched = torch.zeros(nm, dtype=torch.bool, device=DEV)
    for net in (0, 1):
        v = NZ.split_xi(r["xi"][net].double(), A, N)
        for name in NZ.MU:
            mu64 = plan.seg(r["p"][net], name).double()
            ref = mu64 + plan.seg(r["p"][net], NZ.SIGMA[name]).double() * NZ.outer(v, name, mu64.shape)
            got = r["fc32"][net] if name == "wfc" else plan.seg(r["e32"][net], name)
            orc = of32[net] if name == "wfc" else plan.seg(o32[net], name)
            e = ((got.double() - ref).abs() / _ulp32(ref)).max()
            worst = max(worst, float(e))
            assert float(e) <= 1.0, (name, net, float(e))
            assert float(((orc.double() - ref).abs() / _ulp32(ref)).max()) <= 1.0, name
            assert float(((got.double() - orc.double()).abs() / _ulp32(ref)).max()) <= 1.0, name
            if name != "wfc":
                touched[lay.offsets[name]:lay.offsets[name] + mu64.numel()] = True
        # hi (/ lo): the project's split of the fp32 value the kernel itself reported
        w = r["fc32"][net]
        hi = plan.seg(r["ebf"][net, :nm], "wfc")
        hi_ref = w.to(torch.bfloat16)
        assert torch.equal(hi.view(torch.int16), hi_ref.view(torch.int16))
        if split:
            lo = plan.seg(r["ebf"][net, nm:], "wfc")
            lo_ref = (w - hi_ref.float()).to(torch.bfloat16)
            assert torch.equal(lo.view(torch.int16), lo_ref.view(torch.int16))
        # untouched: the fp32 shadow outside heads / biases (conv segments, the wfc range, padding),
        # the bf16 planes outside wfc
        assert bool((r["e32"][net][~touched] == 7.0).all())
        bt = torch.zeros(nm, dtype=torch.bool, device=DEV)
        bt[lay.offsets["wfc"]:lay.offsets["wfc"] + 1024 * 3136] = True
        for plane in range(2 if split else 1):
            assert bool((r["ebf"][net, plane * nm:(plane + 1) * nm][~bt] == 3.0).all())
    print(f"(A, N) = ({A}, {N}) split {split}: max error {worst:.3f} ulp")


@pytest.mark.parametrize("split", [True, False])
def test_noisy_compose_sigma_zero_is_the_existing_cast(split):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    A, N = 3, 7
    r = _compose(A, N, split, 4, zero_sigma=True)
    plan, nm = r["plan"], r["nm"]
    for net in (0, 1):
        mu = plan.seg(r["p"][net], "wfc").contiguous()
        hi = torch.zeros(1024, 3136, device=DEV, dtype=torch.bfloat16)
        lo = torch.zeros_like(hi) if split else None
        HipBackend().cast_bf16(mu, hi, lo)
        torch.cuda.synchronize()
        assert torch.equal(plan.seg(r["ebf"][net, :nm], "wfc").view(torch.int16), hi.view(torch.int16))
        if split:
            assert torch.equal(plan.seg(r["ebf"][net, nm:], "wfc").view(torch.int16), lo.view(torch.int16))
        assert torch.equal(r["fc32"][net], mu)
        for name in ("wv", "bv", "wa", "ba", "bfc"):
            assert torch.equal(plan.seg(r["e32"][net], name), plan.seg(r["p"][net], name))


# ------------------------------------------------------------ 3. sigma gradient
@pytest.mark.parametrize("A,N", SHAPES)
def test_noisy_sigma_grad(A, N):
    from apex_dqn_amd.learner import noisy as NZ
    from apex_dqn_amd.ops.fused_ops import HipBackend
    r = _compose(A, N, False, 9, nnets=1, fc32=False)
    plan, lay = r["plan"], r["lay"]
    gen = torch.Generator().manual_seed(5)
    g0 = (torch.randn(lay.numel, generator=gen) * 1e-2).to(DEV)
    g = g0.clone()
    be = HipBackend()
    be.noisy_sigma_grad(plan, g, r["xi"][0])
    torch.cuda.synchronize()
    first_sigma = lay.offsets["swv"]
    assert torch.equal(g[:first_sigma], g0[:first_sigma])        # mu segments and conv gradients: bit-unchanged
    v = NZ.split_xi(r["xi"][0].double(), A, N)
    sig = torch.zeros(lay.numel, dtype=torch.bool, device=DEV)
    worst = 0.0
    for name in NZ.MU:
        gm = plan.seg(g0, name).double()
        ref = gm * NZ.outer(v, name, gm.shape)
        got = plan.seg(g, NZ.SIGMA[name]).double()
        e = float(((got - ref).abs() / _ulp32(ref)).max())
        worst = max(worst, e)
        assert e <= 1.0, (name, e)
        o = lay.offsets[NZ.SIGMA[name]]
        sig[o:o + gm.numel()] = True
    assert torch.equal(g[first_sigma:][~sig[first_sigma:]], g0[first_sigma:][~sig[first_sigma:]])    # padding
    print(f"(A, N) = ({A}, {N}): sigma gradient max error {worst:.3f} ulp")
    # the optimizer's own norm pass covers the whole flat gradient, sigma included
    n = lay.numel
    p32, vv, mm = r["p"][0].clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pbf = torch.zeros(n, device=DEV, dtype=torch.bfloat16)
    partials, gnorm = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    be.optimizer(p32, g, vv, mm, pbf, 1e-4, 0.95, 1.5e-7, 40.0, True, partials, gnorm)
    torch.cuda.synchronize()
    want = float(g.double().norm())
    assert abs(float(gnorm) - want) <= 1e-5 * want, (float(gnorm), want)
    assert float(g[first_sigma:].double().norm()) > 0.1 * want


# -------------------------------------------------------------- 4. whole step
def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"noisy": True, **rt}})


@pytest.mark.parametrize("N", [1, 51])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_noisy_learner_step_hip_vs_torch_backend(dtype, N):
    """tests/test_gpu_qr.py test_qr_learner_step_hip_vs_torch_backend with noisy layers (the scalar
    head and C51 with 51 atoms) at B = 32: that test's bounds on td_abs, loss_b and the
    per-segment gradient errors, now over the sigma segments too, and its clip-norm identity."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, num_atoms=N)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.N == N and L.noisy and L.split == split and not L._fuse_norm
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, float(L.gnorm), gn)
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout)
    assert torch.equal(res["hip"][2], res["torch"][2])
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    assert {"swv", "sbv", "swa", "sba", "swfc", "sbfc"} <= set(gh)
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} HIP step vs the torch backend, N = {N}):", errs)
    assert max(errs.values()) < 0.2, errs
    for k in ("wv", "wa", "swv", "sbv", "swa", "sba", "swfc", "sbfc"):
        assert float(gt[k].norm()) > 0 and float(gh[k].norm()) > 0, k


# ------------------------------------------------------------------ 5. graphs
def test_noisy_graph_steps_match_eager_steps():
    """steps(8) replaying two 4-update graphs == 8 eager step() calls of a twin (noisy + QR with
    32 quantiles, an lr schedule on), at tests/test_gpu_qr.py's tolerances; the draw left on the
    device is the mirror's for update 7: the index is read inside the replayed graph."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.noisy import gaussians
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res = {}
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, lr_warmup_steps=3, lr_decay_steps=6, lr_end=1e-5,
                   num_atoms=32, dist_head="quantile", learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        u0 = L.update_index()
        if graphs:
            L.steps(8)
            assert L._multi is not None
        else:
            for _ in range(8):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 8 and L.update_index() - u0 == 8
        K = L._nz.K
        for net in (0, 1):
            g_ref = torch.from_numpy(gaussians(L._nz.seed, 7, net, K))
            assert float((_gauss(L.xi[net, :K].cpu()) - g_ref).abs().max()) <= 2e-5, (graphs, net)
        xi = L.xi.clone()
        if graphs:
            assert L.graph_matches_eager() is True
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.S["idx"].clone(), xi)
    assert torch.equal(res[True][3], res[False][3])
    assert torch.equal(res[True][4], res[False][4])                  # the same draws, bit for bit
    o = L.layout.offsets
    assert not torch.equal(res[True][0][o["swfc"]:], torch.full_like(res[True][0][o["swfc"]:], 0.5 / 56))
    for a, b in zip(res[True][:3], res[False][:3]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------- 6. actor
def test_noisy_actor_group_q_values_and_resample():
    """One inference call of a noisy GPU actor group against the fp32 module with the mirror's
    draw for (s = 2 + group, call index // resample), at tests/test_gpu_qr.py's actor q-value
    tolerance (1e-4 absolute; fp32 learner: split kernels); with noisy_actor_resample = 3 calls
    0-2 share one draw and call 3 takes the next."""
    from apex_dqn_amd.actors.gpu_actor import GpuActorGroup
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.envs.vector_envs import make_vec_env
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.noisy import set_module_noise
    from apex_dqn_amd.models.dueling import DuellingDQN
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    E, A, group = 24, 6, 1
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Actor": {"num_actors": E}, "Learner": {"replay_sample_size": 32},
                                "Runtime": {"use_graphs": False, "dtype": "fp32", "noisy": True,
                                            "noisy_actor_resample": 3, "seed": 4}})
    torch.manual_seed(3)
    rp = GpuReplayShard(1000, 1000, 1200, 4, device=DEV)
    L = FusedNatureLearner(cfg, DEV, rp)
    with torch.no_grad():
        for s in ("swv", "sbv", "swa", "sba", "swfc", "sbfc"):
            L.P[s].mul_(4.0)                       # a visible noise term
    env = make_vec_env(cfg.env_backend, cfg.env_conf.name, E, A, seed=0)
    grp = GpuActorGroup(cfg, L, rp, env, E, group=group)
    assert grp.noisy and grp.split and grp._nz.stream0 == 2 + group and grp._nz.every == 3
    rng = np.random.default_rng(5)
    seqs = rp.append_frames(rng.integers(0, 255, (E + 8, 84, 84), dtype=np.uint8))
    payload = np.stack([seqs[i:i + 4] for i in range(E)])
    slots = torch.from_numpy((payload % rp.F).astype(np.int32)).to(DEV)
    frames = rp.gather_frames(slots)
    net = DuellingDQN((4, 84, 84), A, obs_scale=cfg.Runtime.obs_scale, **cfg.head_kw()).to(DEV)
    net.load_state_dict(flat_state(grp))
    grp.eps.zero_()
    draws, qs = [], []
    for call in range(4):
        assert int(grp.ctr) == call
        q, a = grp.policy(payload)
        draws.append(grp.xi[0, :grp._nz.K].clone())
        qs.append(q)
        set_module_noise(net, cfg.Runtime.seed, call // 3, 2 + group)
        with torch.no_grad():
            q_ref = net(frames)[2].double().cpu()
        err = float((torch.from_numpy(q).double() - q_ref).abs().max())
        print(f"call {call}: max |q_actor - q_module| = {err:.2e} (|q| max {float(q_ref.abs().max()):.2e})")
        assert err < 1e-4, (call, err)
        assert np.array_equal(a, q.argmax(1))
    assert torch.equal(draws[0], draws[1]) and torch.equal(draws[1], draws[2]) and not torch.equal(draws[2], draws[3])
    assert np.array_equal(qs[0], qs[2]) and float(np.abs(qs[3] - qs[2]).max()) > 1e-3      # another draw, other q


def flat_state(grp):
    from apex_dqn_amd.models.flat_params import flat_to_reference_state
    return flat_to_reference_state(grp.P, 64)


# ---------------------------------------------------------------- 7. GPU loop
def test_noisy_gpu_loop_lock_step():
    """tests/test_gpu_qr.py test_qr_gpu_loop_lock_step's config with noisy layers on, 40 updates."""
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 20, "q_target_sync_freq": 25},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 20, "use_graphs": True, "num_atoms": 32,
                                            "dist_head": "quantile", "noisy": True}})
    out = train_frames(cfg, DEV, 40, num_envs=16, async_actors=False)
    L, rp = out["learner"], out["replay"]
    torch.cuda.synchronize()
    assert L.N == 32 and L.quantile and L.noisy and L.num_q_updates == 40
    assert out["actors"].noisy and out["actors"].inserted >= 300 + 16 * 20
    live = rp.leaf[rp.leaf != 0]
    assert bool((live > 0).all())
    assert live.numel() >= 300 and bool(torch.isfinite(live).all())
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
    assert np.isfinite(m["noisy_sigma_mean"]) and m["noisy_sigma_mean"] != float(np.float32(0.5 / 56.0))
    q = out["actors"].q
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all()) and float(q.abs().max()) > 0


# ------------------------------------------------------------------ 8. resume
def test_noisy_gpu_resume_matches_uninterrupted_run(tmp_path):
    """Save after 4 updates, load into a fresh learner, 4 more: bit-equal to 8 uninterrupted
    updates (mu, sigma, optimizer state), as tests/test_gpu_opt_schedules.py's resume test
    demands of the plain net."""
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

    def replay():
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=5)
        fill_replay(rp, 1500, seed=2)
        return rp

    cfg = _cfg(32, use_graphs=True, learner={"q_target_sync_freq": 3})
    rp = replay()
    torch.manual_seed(0)
    L = FusedNatureLearner(cfg, DEV, rp)
    for _ in range(4):
        L.step()
    torch.cuda.synchronize()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(4):
        L.step()
    torch.cuda.synchronize()
    rp2 = replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    torch.manual_seed(9)
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.noisy and L2.num_q_updates == L2.update_index() == 4
    for _ in range(4):
        L2.step()
    torch.cuda.synchronize()
    o = L.layout.offsets
    assert not torch.equal(L.p32[o["swfc"]:], torch.full_like(L.p32[o["swfc"]:], float(np.float32(0.5 / 56.0))))
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.S["weights"], L2.S["weights"]), (L.xi, L2.xi)):
        assert torch.equal(a, b)
