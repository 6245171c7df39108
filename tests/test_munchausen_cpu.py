"""Munchausen-DQN target on the CPU: ``munchausen_loss`` by hand and in its limits, the fused
learner's hand-written backward against autograd, the row plan of the sampler, the config
refusals, and the torch learner / inline loop with the target."""
import math
import os

import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.losses import munchausen_loss, munchausen_targets, tau_log_policy
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.flat_params import flat_to_reference_state
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


def t64(x):
    return torch.tensor(x, dtype=D)


# ------------------------------------------------------------------------ loss
def _by_hand(q_on, g0, g1, a, R, Gm, w, alpha, tau, clip, loss, kappa):
    """One sample in plain Python floats, from the issue's definition: returns
    (loss_b, |delta|, tau ln pi(a | g0), bonus, vsoft, dloss_b / dq_on[a])."""
    m0 = max(g0)
    tl = (g0[a] - m0) - tau * math.log(sum(math.exp((x - m0) / tau) for x in g0))
    bonus = alpha * min(max(tl, clip), 0.0)
    m1 = max(g1)
    z1 = sum(math.exp((x - m1) / tau) for x in g1)
    pi1 = [math.exp((x - m1) / tau) / z1 for x in g1]
    tl1 = [(x - m1) - tau * math.log(z1) for x in g1]
    vsoft = sum(p * (x - t) for p, x, t in zip(pi1, g1, tl1))          # the expectation form
    d = R + bonus + Gm * vsoft - q_on[a]
    if loss == "huber" and abs(d) > kappa:
        l, dl = kappa * (abs(d) - 0.5 * kappa), math.copysign(kappa, d)
    else:
        l, dl = 0.5 * d * d, d
    return w * l, abs(d), tl, bonus, vsoft, -w * dl


HAND = dict(
    # row 0: the clip is active (tau ln pi ~ -5 < -1); row 1: strictly inside (-1, 0); row 2: terminal;
    # row 3: equal q's at S_t, tau ln pi = -tau ln 3 exactly
    q_on=[[0.3, -0.2, 0.1], [1.0, 0.4, 0.2], [0.0, 0.5, -0.5], [0.25, 0.5, 0.75]],
    g0=[[0.0, 5.0, 0.0], [1.0, 1.2, 0.5], [0.3, 0.1, 0.2], [2.0, 2.0, 2.0]],
    g1=[[0.5, 0.2, 0.1], [3.0, 0.0, 2.9], [7.0, 8.0, 9.0], [0.1, 0.1, 0.4]],
    a=[0, 1, 2, 1], R=[1.0, -0.5, 2.0, 0.0], Gm=[0.97, 0.97, 0.0, 0.5], w=[1.0, 0.5, 2.0, 0.25])


@pytest.mark.parametrize("loss", ["huber", "mse"])
def test_loss_by_hand(loss):
    alpha, tau, clip, kappa = 0.9, 0.5, -1.0, 1.0
    h = HAND
    rows = [_by_hand(h["q_on"][b], h["g0"][b], h["g1"][b], h["a"][b], h["R"][b], h["Gm"][b], h["w"][b], alpha, tau, clip,
                     loss, kappa) for b in range(4)]
    # the four cases are what they claim to be
    assert rows[0][2] < clip and rows[0][3] == alpha * clip
    assert clip < rows[1][2] < 0.0 and rows[1][3] == alpha * rows[1][2]
    assert h["Gm"][2] == 0.0 and abs(rows[2][1] - abs(h["R"][2] + rows[2][3] - h["q_on"][2][2])) < 1e-15
    assert abs(rows[3][2] + tau * math.log(3.0)) < 1e-15
    q = t64(h["q_on"]).requires_grad_(True)
    lv, td = munchausen_loss(q, t64(h["g0"]), t64(h["g1"]), torch.tensor(h["a"]), t64(h["R"]), t64(h["Gm"]), t64(h["w"]),
                             alpha, tau, clip, loss, kappa)
    assert lv.dtype == D and td.dtype == D
    assert abs(float(lv.detach()) - sum(r[0] for r in rows) / 4) < 1e-13
    torch.testing.assert_close(td, t64([r[1] for r in rows]), rtol=0, atol=1e-13)
    lv.backward()
    want = torch.zeros(4, 3, dtype=D)
    for b in range(4):
        want[b, h["a"][b]] = rows[b][5] / 4            # through q_on[a] only
    torch.testing.assert_close(q.grad, want, rtol=0, atol=1e-13)
    T, bonus, vsoft = munchausen_targets(t64(h["g0"]), t64(h["g1"]), torch.tensor(h["a"]), t64(h["R"]), t64(h["Gm"]),
                                         alpha, tau, clip)
    torch.testing.assert_close(bonus, t64([r[3] for r in rows]), rtol=0, atol=1e-13)
    torch.testing.assert_close(vsoft, t64([r[4] for r in rows]), rtol=0, atol=1e-13)
    # no weights: w = 1
    lv1, _ = munchausen_loss(q.detach(), t64(h["g0"]), t64(h["g1"]), torch.tensor(h["a"]), t64(h["R"]), t64(h["Gm"]),
                             None, alpha, tau, clip, loss, kappa)
    assert abs(float(lv1) - sum(r[0] / w for r, w in zip(rows, h["w"])) / 4) < 1e-13


def _gapped(B, A, gap, g):
    """[B, A] q-values whose entries differ pairwise by at least ``gap`` in every row."""
    base = torch.rand(B, 1, generator=g, dtype=D) * 2 - 1
    steps = gap * (1.0 + torch.rand(B, A, generator=g, dtype=D))
    q = base + torch.cumsum(steps, 1)
    perm = torch.stack([torch.randperm(A, generator=g) for _ in range(B)])
    return q.gather(1, perm)


def test_limit_alpha_zero_small_tau_is_the_hard_max():
    g = torch.Generator().manual_seed(0)
    B, A = 16, 5
    g0, g1, q = _gapped(B, A, 0.1, g), _gapped(B, A, 0.1, g), torch.randn(B, A, generator=g, dtype=D)
    a = torch.randint(0, A, (B,), generator=g)
    R, Gm = torch.randn(B, generator=g, dtype=D), torch.full((B,), 0.97, dtype=D)
    T, bonus, vsoft = munchausen_targets(g0, g1, a, R, Gm, 0.0, 1e-3, -1.0)
    assert float(bonus.abs().max()) == 0.0
    torch.testing.assert_close(T, R + Gm * g1.max(1).values, rtol=0, atol=1e-12)
    _, td = munchausen_loss(q, g0, g1, a, R, Gm, None, 0.0, 1e-3, -1.0)
    torch.testing.assert_close(td, (R + Gm * g1.max(1).values - q.gather(1, a[:, None]).squeeze(1)).abs(), rtol=0,
                               atol=1e-12)


def test_limit_one_action():
    g = torch.Generator().manual_seed(1)
    g0, g1 = torch.randn(7, 1, generator=g, dtype=D), torch.randn(7, 1, generator=g, dtype=D)
    R, Gm = torch.randn(7, generator=g, dtype=D), torch.full((7,), 0.9, dtype=D)
    T, bonus, vsoft = munchausen_targets(g0, g1, torch.zeros(7, dtype=torch.long), R, Gm, 0.9, 0.03, -1.0)
    assert float(bonus.abs().max()) == 0.0
    assert torch.equal(vsoft, g1[:, 0]) and torch.equal(T, R + Gm * g1[:, 0])


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_no_nan_or_inf_with_huge_gaps(dt):
    tau = 0.03
    gap = 1e4 / tau
    g0 = torch.tensor([[0.0, gap, 2 * gap], [gap, 0.0, -gap], [0.0, 0.0, gap]], dtype=dt)
    g1 = torch.tensor([[gap, 0.0, -gap], [0.0, 2 * gap, gap], [-gap, 0.0, 0.0]], dtype=dt)
    a = torch.tensor([0, 0, 1])
    R, Gm = torch.zeros(3, dtype=dt), torch.ones(3, dtype=dt)
    T, bonus, vsoft = munchausen_targets(g0, g1, a, R, Gm, 0.9, tau, -1.0)
    for t in (T, bonus, vsoft):
        assert bool(torch.isfinite(t).all())
    # every non-max exp underflows: clipped bonus off the maximum, none on it; vsoft = max g1 (row 2: two maxima)
    torch.testing.assert_close(bonus, torch.tensor([-0.9, 0.0, -0.9], dtype=dt), rtol=0, atol=0)
    want = g1.max(1).values + torch.tensor([0.0, 0.0, tau * math.log(2.0)], dtype=dt)
    torch.testing.assert_close(vsoft, want, rtol=1e-6 if dt == torch.float32 else 1e-15, atol=0)
    q = torch.zeros(3, 3, dtype=dt, requires_grad=True)
    lv, td = munchausen_loss(q, g0, g1, a, R, Gm, None, 0.9, tau, -1.0)
    lv.backward()
    assert math.isfinite(float(lv)) and bool(torch.isfinite(td).all()) and bool(torch.isfinite(q.grad).all())


def test_expectation_equals_closed_form():
    g = torch.Generator().manual_seed(2)
    for tau in (0.03, 0.5, 1.0):
        g1 = torch.randn(64, 6, generator=g, dtype=D) * 0.3
        _, _, vsoft = munchausen_targets(g1, g1, torch.zeros(64, dtype=torch.long), torch.zeros(64, dtype=D),
                                         torch.ones(64, dtype=D), 0.9, tau, -1.0)
        m = g1.max(1).values
        closed = m + tau * torch.log(torch.exp((g1 - m[:, None]) / tau).sum(1))
        torch.testing.assert_close(vsoft, closed, rtol=0, atol=1e-12)
        # and tau ln pi is a normalised log-policy
        torch.testing.assert_close((tau_log_policy(g1, tau) / tau).exp().sum(1), torch.ones(64, dtype=D), rtol=0,
                                   atol=1e-12)


# -------------------------------------------------------------- fused learner
def _setup(A=4, B=6, **rt):
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": B},
                                "Runtime": {"grad_clip": 40.0, "network": "nature64", "presample": False,
                                            "munchausen": True, **rt}})
    rp = GpuReplayShard(400, 400, 600, 4, device="cpu")
    rng = np.random.default_rng(0)
    seqs = rp.append_frames(rng.integers(0, 255, (300, 84, 84), dtype=np.uint8))
    K = 200
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    nx = np.stack([seqs[i + 3:i + 7] for i in range(K)])
    g = np.full(K, 0.97)
    g[::5] = 0.0
    rp.insert(dict(S_t=st, S_tpn=nx, A_t=rng.integers(0, A, K), R=rng.normal(size=K) * 3, Gamma=g,
                   priority=rng.random(K)))
    return cfg, rp


@pytest.mark.parametrize("loss,noisy", [("huber", False), ("mse", False), ("huber", True)])
def test_fused_backward_matches_autograd(loss, noisy):
    """One update's flat gradient against autograd through DuellingDQN and munchausen_loss, with the
    bounds of tests/test_qr_cpu.py test_fused_backward_matches_autograd."""
    cfg, rp = _setup(loss=loss, noisy=noisy)
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.munchausen and L.N == 1 and L._rows_first == L.B == 6 and not L._defer_fc_epilogue
    assert L.dhead.shape == (6, 5) and L.mdqn_aux.shape == (6, 2)
    T = TorchLearner(cfg, "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    # the target net differs from the online net, so a swapped row block would show
    with torch.no_grad():
        for p in T.Q_target.parameters():
            p.mul_(1.25)
    from apex_dqn_amd.models.flat_params import reference_state_to_flat
    from apex_dqn_amd.ops.fused_ops import split_into
    reference_state_to_flat(T.Q_target.state_dict(), L.T)
    split_into(L.t32, L.tbf, L.tbf_lo)
    L._target_changed()
    L._seg1()
    L._seg2()
    if noisy:
        from apex_dqn_amd.learner import noisy as NZ
        T.Q.set_noise(NZ.split_xi(L.xi[0], L.A, 1))
        T.Q_target.set_noise(NZ.split_xi(L.xi[1], L.A, 1))
    B, S = L.B, L.S
    assert torch.equal(L.frames[2 * B:], L.frames[:B])
    batch = dict(S_t=L.frames[:B], S_tpn=L.frames[B:2 * B], A_t=S["act"], R=S["rew"], Gamma=S["gam"],
                 weights=S["weights"])
    lref, td = T.compute_loss_and_priorities(batch)
    T.optimizer.zero_grad()
    lref.backward()
    assert abs(float(lref) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref)))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    names = dict(T.Q.named_parameters())
    assert set(gf) == set(names)
    for k, p in names.items():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")
    assert float(gf["value.weight"].norm()) > 0 and float(gf["advantage.weight"].norm()) > 0
    assert any(k.endswith("_sigma") for k in gf) == noisy
    m = L.last_metrics()
    tm = T.last_metrics()
    assert m["munchausen_bonus_mean"] <= 0.0
    assert abs(m["munchausen_bonus_mean"] - tm["munchausen_bonus_mean"]) < 1e-5
    assert abs(m["soft_value_mean"] - tm["soft_value_mean"]) < 1e-5 * max(1.0, abs(tm["soft_value_mean"]))


def test_fused_step_updates_params_and_priorities():
    cfg, rp = _setup()
    L = FusedNatureLearner(cfg, "cpu", rp)
    p0, leaf0 = L.p32.clone(), rp.leaf.clone()
    L.step()
    L.step()
    assert not torch.equal(p0, L.p32) and L.num_q_updates == 2
    assert not torch.equal(leaf0[L.S["idx"]], rp.leaf[L.S["idx"]]) and bool(torch.isfinite(rp.leaf).all())


@pytest.mark.parametrize("presample", [False, True])
def test_row_plan(presample):
    for on in (True, False):
        cfg, rp = _setup(munchausen=on, presample=presample)
        L = FusedNatureLearner(cfg, "cpu", rp)
        B = L.B
        if presample:
            L.step()               # the optimizer call drew the next batch
        else:
            L._sample()
        idx = L.S["idx"]
        assert torch.equal(L.slots[:B], rp.obs[idx]) and torch.equal(L.slots[B:2 * B], rp.nxt[idx])
        assert L.S["nxt"].data_ptr() == L.slots[B:2 * B].data_ptr()
        assert not torch.equal(L.slots[:B], L.slots[B:2 * B])
        assert torch.equal(L.slots[2 * B:], L.slots[:B] if on else L.slots[B:2 * B])
        assert L._rows_first == (B if on else 2 * B)


def test_sampler_obs2_is_optional_and_changes_nothing():
    _, rp = _setup()
    outs = []
    for with_obs2 in (True, False):
        rp.ctr.fill_(5)
        out = rp.alloc_sample_buffers(6)
        o2 = torch.full((6, 4), -7, dtype=torch.int32)
        n2 = torch.full((6, 4), -7, dtype=torch.int32)
        rp.sample(6, out=out, nxt2=n2, **({"obs2": o2} if with_obs2 else {}))
        assert torch.equal(n2, out["nxt"])
        assert torch.equal(o2, out["obs"]) if with_obs2 else bool((o2 == -7).all())
        outs.append(out)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ---------------------------------------------------------------------- config
def _cfg(net=None, **rt):
    ss = [4] if net == "mlp" else [4, 84, 84]
    return ApexConfig.from_dict({"env_conf": {"state_shape": ss, "action_dim": 4, "name": "Synthetic"}, "Runtime": rt})


@pytest.mark.parametrize("rt,key", [
    (dict(munchausen=True, num_atoms=51), "Runtime.munchausen"),
    (dict(munchausen=True, num_atoms=32, dist_head="quantile"), "Runtime.munchausen"),
    (dict(munchausen=True, network="impala"), "Runtime.munchausen"),
    (dict(munchausen=True, world_size=2), "Runtime.munchausen"),
    (dict(munchausen=True, force_dp=True), "Runtime.munchausen"),
    (dict(munchausen="yes"), "Runtime.munchausen"),
    (dict(munchausen_alpha=1.5), "Runtime.munchausen_alpha"),
    (dict(munchausen_alpha=-0.1), "Runtime.munchausen_alpha"),
    (dict(munchausen_tau=0.0), "Runtime.munchausen_tau"),
    (dict(munchausen_tau=-1.0), "Runtime.munchausen_tau"),
    (dict(munchausen_clip=0.0), "Runtime.munchausen_clip"),
    (dict(munchausen_clip=1.0), "Runtime.munchausen_clip"),
])
def test_config_refusals(rt, key):
    with pytest.raises(ValueError, match=key):
        _cfg(**rt)


def test_config_defaults_round_trip_and_file():
    c = _cfg()
    rt = c.Runtime
    assert (rt.munchausen, rt.munchausen_alpha, rt.munchausen_tau, rt.munchausen_clip) == (False, 0.9, 0.03, -1.0)
    m = _cfg(munchausen=True, noisy=True, munchausen_alpha=0.0, munchausen_tau=1.0, munchausen_clip=-2.0)
    assert m.munchausen_kw() == dict(alpha=0.0, tau=1.0, clip=-2.0) and m.Runtime.noisy
    assert ApexConfig.from_dict(m.to_dict()).to_dict() == m.to_dict()
    assert _cfg("mlp", munchausen=True).network == "mlp"
    f = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_munchausen.json"))
    assert f.Runtime.munchausen and f.Runtime.num_atoms == 1 and f.network == "nature64"
    o = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu.json"), ["Runtime.munchausen=true"])
    assert o.Runtime.munchausen is True


def test_learners_without_the_target_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    cfg, rp = _setup()
    with pytest.raises(ValueError, match="Runtime.munchausen"):
        GraphLearner(cfg, "cpu", rp)

    class Comm:                      # a second rank: the data-parallel step
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="Runtime.munchausen"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


def test_checkpoint_loads_across_the_setting(tmp_path):
    cfg, rp = _setup()
    L = FusedNatureLearner(cfg, "cpu", rp)
    L.step()
    path = str(tmp_path / "m.pt")
    L.save(path)
    cfg2, rp2 = _setup(munchausen=False)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    assert not L2.munchausen and L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m)):
        assert torch.equal(a, b)
    assert L2._last_ckpt["config"]["Runtime"]["munchausen"] is True


# --------------------------------------------------------------- torch learner
def test_mlp_torch_learner_takes_updates():
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 1000},
                                "Runtime": {"munchausen": True, "lr": 1e-3}})
    T = TorchLearner(cfg, "cpu")
    g = torch.Generator().manual_seed(3)
    B = 32
    batch = dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                 A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g) * 3,
                 Gamma=torch.full((B,), 0.97), weights=torch.rand(B, generator=g) + 0.5)
    for _ in range(3):
        out = T.step(batch)
        assert np.isfinite(out["loss"]) and out["td_abs"].shape == (B,) and np.isfinite(out["td_abs"]).all()
        assert out["munchausen_bonus_mean"] <= 0.0 and np.isfinite(out["soft_value_mean"])
    assert T.num_q_updates == 3
    # the loss is munchausen_loss of learner/losses.py on this batch
    with torch.no_grad():
        ref, _ = munchausen_loss(T.Q(batch["S_t"])[2], T.Q_target(batch["S_t"])[2], T.Q_target(batch["S_tpn"])[2],
                                 batch["A_t"], batch["R"], batch["Gamma"], batch["weights"], 0.9, 0.03, -1.0, "huber", 1.0)
        now, _ = T.compute_loss_and_priorities(batch)
    assert float(ref) == float(now)


def test_inline_cartpole_runs_with_the_flag():
    from apex_dqn_amd.runtime.loops import train_inline
    cfg = ApexConfig.load(os.path.join(ROOT, "configs", "cartpole.json"), ["Runtime.munchausen=true"])
    assert cfg.Runtime.munchausen and cfg.network == "mlp"
    out = train_inline(cfg, 50)
    T = out["learner"]
    assert T.num_q_updates == 50 and len(out["losses"]) == 50 and np.isfinite(out["losses"]).all()
    m = T.last_metrics()
    assert m["munchausen_bonus_mean"] <= 0.0 and np.isfinite(m["soft_value_mean"])
