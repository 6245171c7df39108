"""Histogram-loss (HL-Gauss) target of the categorical head on the GPU: csrc/c51_head.hip ``hlg_head_kernel``
against the fp64 torch oracle (``TorchBackend.hlg_head``, tests/hlg_fixtures.py), the launcher's refusals, the
whole step against the torch backend, graph capture, resume, the GPU loop and an actor group."""
import hlg_fixtures as F
import numpy as np
import pytest
import torch
from head_fixtures import fill_replay

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
VMIN, VMAX = F.VMIN, F.VMAX


def _run_hip(B, A, N, split=False, case="plain", sigma=F.SIGMA, rescale_eps=None, every=False, vmin=VMIN, vmax=VMAX):
    """``hlg_head_kernel`` + ``head_wgrad`` on the problem's inputs; ``every``: q_out, the zeroed region and the
    IS statistic with its count are passed too (the lo planes come with ``split``)."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be = HipBackend()
    fx = F.fixture(B, A, N, split)
    rew, gam, isw = F.case_inputs(fx, case)
    dev = lambda t: None if t is None else t.to(DEV)                     # noqa: E731
    Hon, Htg, Hon_lo, Htg_lo = dev(fx["Hon"]), dev(fx["Htg"]), dev(fx["Hon_lo"]), dev(fx["Htg_lo"])
    Pon, Ptg = {k: dev(v) for k, v in fx["Pon"].items()}, {k: dev(v) for k, v in fx["Ptg"].items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16)
    dH_lo = torch.zeros_like(dH) if split else None
    dhead = torch.full((B, (A + 1) * N), 7.0, device=DEV)
    q = torch.zeros(B, A, device=DEV)
    flat = torch.full((sum(v.numel() for v in Pon.values()),), 3.0, device=DEV)     # zeroed by the head launch
    gr, o = {}, 0
    for k in ("wv", "bv", "wa", "ba"):
        gr[k] = flat[o:o + Pon[k].numel()].view(Pon[k].shape)
        o += Pon[k].numel()
    stat = (torch.full((1,), F.WSCALE, device=DEV), torch.full((1,), -1.0, dtype=torch.float64, device=DEV),
            torch.zeros((), dtype=torch.int64, device=DEV))
    be.hlg_head(Hon, Htg, Pon, Ptg, dev(fx["act"]), dev(rew), dev(gam), dev(isw), N, vmin, vmax, sigma, 1.0 / B, td, loss,
                dH, dhead, q_out=q, zero=flat, lo=(Hon_lo, Htg_lo, dH_lo) if split else None,
                isn=stat if every else None, rescale_eps=rescale_eps)
    torch.cuda.synchronize()
    zeroed = bool((flat == 0).all())
    be.head_wgrad(Hon, dhead, gr, Hon_lo=Hon_lo)
    torch.cuda.synchronize()
    dHj = dH.double() + (dH_lo.double() if split else 0.0)
    return dict(td=td.cpu(), loss=loss.cpu(), dH=dHj.cpu(), dhead=dhead.cpu(), q=q.cpu(),
                g={k: v.cpu() for k, v in gr.items()}, zeroed=zeroed, isn=float(stat[1].cpu()), count=int(stat[2].cpu()))


def _check(prob, **kw):
    r = F.oracle(*prob)
    h = _run_hip(*prob, **kw)
    print(prob, f"gap {r['gap']:.2e}", {k: f"{v:.2e}" for k, v in F.max_errors(h, r).items()})
    F.compare(h, r)
    assert h["zeroed"]
    return h, r


# --------------------------------------------------------- 1. kernel vs oracle
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", F.SHAPES + [F.FRAME_EDGE])
def test_hlg_head_kernel_vs_fp64_oracle(B, A, N, split):
    """bf16 single plane and split hi / lo inputs at sigma_ratio = 0.75.  B = 5: a ragged last block; (3, 3, 2):
    the smallest head and the widest Gaussian (delta = 20, sigma = 15); (3, 2, 2): tests/hlg_fixtures.py
    FRAME_EDGE."""
    h, r = _check((B, A, N, split, "plain", F.SIGMA, None))
    assert r["gap"] >= 1e-3, r["gap"]         # no near-tie in the online argmax: every sample is compared


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("sigma", [0.25, 2.0])
def test_hlg_head_kernel_other_sigma_ratios(sigma, split):
    _check((64, 4, 51, split, "plain", sigma, None))


def test_hlg_head_every_optional_argument_at_once():
    """q_out, the zeroed region, the three lo planes, the IS weights and the IS statistic with its output and its
    row count, all given, at (3, 3, 2): two blocks, the second with one live row.  Every member of ``HlgArgs`` the
    launch passes is read or written through, so a member at the wrong offset shows as a wrong number.  The
    statistic is max(isw) / 2 formed in fp64 from the same fp32 weights, and the count an integer: both equal
    the oracle's exactly."""
    B, A, N = 3, 3, 2
    h, r = _check((B, A, N, True, "plain", F.SIGMA, None), every=True)
    fx = F.fixture(B, A, N, True)
    assert r["count"] == B and h["count"] == r["count"]
    assert r["isn"] == float(fx["isw"].max().double() / F.WSCALE) and h["isn"] == r["isn"]


# ------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("case", F.EDGE_CASES)
def test_hlg_head_edge_cases(case):
    """Targets clamped onto either end (the row is the truncated Gaussian there, not one-hot, and td_abs = |v_max
    - q| / |v_min - q|), all-terminal batches and weights off.  sum_i m_i = 1 shows as sum_i d v[i] = w grad_scale
    (sum p - sum m) = 0, bounded as in tests/test_gpu_c51.py: (N + 3) fp32 roundings of the two unit sums, 54 x
    2^-23 = 6.5e-6 < 1e-5, times w grad_scale <= grad_scale."""
    B, A, N = F.EDGE
    h, r = _check((B, A, N, False, case, F.SIGMA, None))
    fx = F.fixture(B, A, N)
    assert float(h["dhead"][:, :N].sum(1).abs().max()) <= 1e-5 / B
    if case in ("rew_hi", "rew_lo"):
        from apex_dqn_amd.learner.losses import hl_gauss_target
        end = VMAX if case == "rew_hi" else VMIN
        m = hl_gauss_target(torch.full((B,), end, dtype=torch.float64), VMIN, VMAX, N, F.SIGMA)
        assert 0.5 < float(m.max()) < 0.9                       # not one-hot
        torch.testing.assert_close(h["loss"], (-fx["isw"].double() * (m * r["lp"]).sum(-1)).float(), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(h["td"], (end - r["q"][torch.arange(B), fx["act"].long()]).abs().float(),
                                   rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------ 3. value rescaling
def test_hlg_head_value_rescale_instantiation():
    """``hlg_head_kernel<true>``: y = clamp(T(R, Gamma, q_target[a*])) at eps = 1e-3, split inputs."""
    h, r = _check((64, 4, 51, True, "plain", F.SIGMA, F.EPS))
    plain = F.oracle(64, 4, 51, True, "plain", F.SIGMA, None)
    assert float((r["td"] - plain["td"]).abs().max()) > 0.1     # (another target than the plain kernel's)


# ------------------------------------------------------------ 4. refusals
def test_launcher_refuses_wrong_arguments():
    """Wrong arguments are refused on the host (hipErrorInvalidValue from ``apex_hlg_head``): nothing launches."""
    for kw in (dict(sigma=0.0), dict(sigma=-0.75), dict(sigma=float("inf")), dict(sigma=float("nan")),
               dict(vmin=3.0, vmax=3.0), dict(vmin=1.0, vmax=-1.0)):
        with pytest.raises(RuntimeError, match="hlg_head"):
            _run_hip(3, 3, 2, **kw)
    torch.cuda.synchronize()


# -------------------------------------------------------------- 5. whole step
def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"num_atoms": 51, "dist_head": "hl_gauss", **rt}})


@pytest.mark.parametrize("dtype,rt", [("bf16", {}), ("fp32", {}), ("bf16", {"noisy": True})])
def test_hlg_learner_step_hip_vs_torch_backend(dtype, rt):
    """tests/test_gpu_c51.py test_c51_learner_step_hip_vs_torch_backend under the histogram loss at B = 32, in the
    bf16-operand mode and the fp32 (split) mode and with noisy layers, with that test's bounds."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, **rt)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.N == 51 and L.cfg.hl_gauss and L.split == split and L.noisy == bool(rt.get("noisy"))
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
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} {rt} HIP step vs the torch backend):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


def test_graph_of_four_updates_is_bit_identical_to_four_eager_steps():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res = {}
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, optimizer="adam", target_ema_rate=0.01,
                   learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        if graphs:
            L.steps(4)
            assert L._multi is not None
        else:
            for _ in range(4):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 4
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.S["idx"].clone(), L.td_abs.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_gpu_resume_is_bit_identical(tmp_path):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

    def replay():
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=5)
        fill_replay(rp, 1500, seed=2)
        return rp
    cfg = _cfg(32, use_graphs=True, graph_steps=4, learner={"q_target_sync_freq": 3})
    rp = replay()
    torch.manual_seed(0)
    L = FusedNatureLearner(cfg, DEV, rp)
    for _ in range(3):
        L.step()
    torch.cuda.synchronize()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(3):
        L.step()
    torch.cuda.synchronize()
    rp2 = replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    assert d["Runtime"]["dist_head"] == "hl_gauss"
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.num_q_updates == 3 and L2.cfg.hl_gauss
    for _ in range(3):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.td_abs, L2.td_abs)):
        assert torch.equal(a, b)
    cat = ApexConfig.from_dict({**d, "Runtime": {**d["Runtime"], "dist_head": "categorical"}})
    with pytest.raises(ValueError, match="dist_head"):
        FusedNatureLearner(cat, DEV, replay()).load(ck)


# ---------------------------------------------------------------- 6. GPU loop, actors
def test_hlg_gpu_loop_lock_step_on_fake_ale():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "PongNoFrameskip-v4"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 20, "q_target_sync_freq": 25},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 20, "use_graphs": True, "num_atoms": 51,
                                            "dist_head": "hl_gauss", "env_backend": "fake_ale"}})
    out = train_frames(cfg, DEV, 40, num_envs=16, async_actors=False)
    L, rp = out["learner"], out["replay"]
    torch.cuda.synchronize()
    assert L.N == 51 and L.cfg.hl_gauss and L.num_q_updates == 40
    assert out["actors"].inserted >= 300 + 16 * 20
    live = rp.leaf[rp.leaf != 0]
    assert bool((live > 0).all())
    assert live.numel() >= 300 and bool(torch.isfinite(live).all())
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
    q = out["actors"].q
    assert bool(torch.isfinite(q).all()) and 0 < float(q.abs().max()) <= VMAX + 1e-3


def test_actor_group_q_is_the_categorical_groups():
    """An actor group under "hl_gauss" runs ``c51_actor_head_kernel``: on the same weights its q and greedy actions
    are bit-equal to a "categorical" group's."""
    from apex_dqn_amd.actors.gpu_actor import GpuActorGroup
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.envs.vector_envs import make_vec_env
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    E, A = 24, 6
    out, p32 = {}, None
    for kind in ("hl_gauss", "categorical"):
        cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                    "Actor": {"num_actors": E}, "Learner": {"replay_sample_size": 32},
                                    "Runtime": {"use_graphs": False, "num_atoms": 51, "dist_head": kind, "seed": 4}})
        torch.manual_seed(3)
        rp = GpuReplayShard(1000, 1000, 1200, 4, device=DEV)
        L = FusedNatureLearner(cfg, DEV, rp)
        if p32 is None:
            p32 = L.p32.clone()
        assert torch.equal(L.p32, p32)                 # the same initial weights under either kind
        env = make_vec_env(cfg.env_backend, cfg.env_conf.name, E, A, seed=0)
        grp = GpuActorGroup(cfg, L, rp, env, E)
        seqs = rp.append_frames(np.random.default_rng(5).integers(0, 255, (E + 8, 84, 84), dtype=np.uint8))
        payload = np.stack([seqs[i:i + 4] for i in range(E)])
        grp.eps.zero_()
        q, a = grp.policy(payload)
        torch.cuda.synchronize()
        out[kind] = (np.array(q, copy=True), np.array(a, copy=True))
    assert np.array_equal(out["hl_gauss"][0], out["categorical"][0]) and np.abs(out["hl_gauss"][0]).max() > 0
    assert np.array_equal(out["hl_gauss"][1], out["categorical"][1])
