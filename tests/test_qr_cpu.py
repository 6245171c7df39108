"""Quantile-regression (QR-DQN) dueling head on the CPU: the quantile Huber loss by hand, the
module and flat layout, the fused learner's hand-written backward against autograd, the
config refusals, checkpoints, and the torch learner training on a fixed batch."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.losses import quantile_huber_loss, quantile_huber_terms
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.dueling import REFERENCE_KEYS, DuellingDQN, build_network
from apex_dqn_amd.models.flat_params import (FlatLayout, flat_to_reference_state, nature_segments,
                                             reference_state_to_flat)
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard


# ------------------------------------------------------------------------ loss
def _one_action(theta, T, kappa, w=None, R=0.0, G=1.0):
    """quantile_huber_loss of one sample with one action: theta [N] online, T = R + G target."""
    th = torch.tensor([[theta]], dtype=torch.float64, requires_grad=True)
    tg = torch.tensor([[T]], dtype=torch.float64)
    loss, td = quantile_huber_loss(th, torch.zeros(1, 1, dtype=torch.float64), tg, torch.zeros(1, dtype=torch.long),
                                   torch.tensor([R], dtype=torch.float64), torch.tensor([G], dtype=torch.float64),
                                   kappa, None if w is None else torch.tensor([w], dtype=torch.float64))
    return th, loss, td


def test_loss_and_gradient_by_hand():
    """N = 2, kappa = 1, w = 1, theta = (0, 1), T = (0.5, 3): tau = (1/4, 3/4);
    i = 0: u = (0.5, 3), L = (0.125, 2.5), both u >= 0 -> 0.25 * 2.625 / 2 = 0.328125;
    i = 1: u = (-0.5, 2), L = (0.125, 1.5), weights (0.25, 0.75) -> 1.15625 / 2 = 0.578125."""
    th, loss, td = _one_action([0.0, 1.0], [0.5, 3.0], 1.0)
    assert abs(float(loss.detach()) - 0.90625) < 1e-15
    loss.backward()
    torch.testing.assert_close(th.grad[0, 0], torch.tensor([-0.1875, -0.3125], dtype=torch.float64), rtol=0, atol=1e-15)
    assert abs(float(td) - abs(1.75 - 0.5)) < 1e-15
    rho, c = quantile_huber_terms(torch.tensor([[0.0, 1.0]], dtype=torch.float64),
                                  torch.tensor([[0.5, 3.0]], dtype=torch.float64), 1.0)
    torch.testing.assert_close(rho[0], torch.tensor([0.328125, 0.578125], dtype=torch.float64), rtol=0, atol=1e-15)
    torch.testing.assert_close(c[0], torch.tensor([0.1875, 0.3125], dtype=torch.float64), rtol=0, atol=1e-15)
    # an IS weight scales loss and gradient
    th2, loss2, _ = _one_action([0.0, 1.0], [0.5, 3.0], 1.0, w=0.5)
    loss2.backward()
    assert abs(float(loss2.detach()) - 0.453125) < 1e-15
    torch.testing.assert_close(th2.grad, 0.5 * th.grad, rtol=0, atol=1e-15)


def test_large_kappa_is_the_quadratic_form():
    g = torch.Generator().manual_seed(0)
    B, N, kappa = 6, 9, 50.0
    th = torch.randn(B, N, generator=g, dtype=torch.float64)
    T = torch.randn(B, N, generator=g, dtype=torch.float64) * 2
    u = T[:, None, :] - th[:, :, None]                                   # [B, i, j]
    assert float(u.abs().max()) < kappa
    tau = (2 * torch.arange(N, dtype=torch.float64) + 1) / (2 * N)
    ref = ((tau[None, :, None] - (u < 0).double()).abs() * 0.5 * u * u).mean(-1) / kappa
    rho, c = quantile_huber_terms(th, T, kappa)
    torch.testing.assert_close(rho, ref, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(c, ((tau[None, :, None] - (u < 0).double()).abs() * u).mean(-1) / kappa,
                               rtol=1e-13, atol=1e-15)


def test_terminal_rows_ignore_the_target_net():
    g = torch.Generator().manual_seed(1)
    B, A, N = 5, 3, 4
    th = torch.randn(B, A, N, generator=g, dtype=torch.float64)
    qn = torch.randn(B, A, generator=g, dtype=torch.float64)
    act = torch.randint(0, A, (B,), generator=g)
    R = torch.randn(B, generator=g, dtype=torch.float64)
    zero = torch.zeros(B, dtype=torch.float64)
    outs = [quantile_huber_loss(th, qn, torch.randn(B, A, N, generator=g, dtype=torch.float64) * s, act, R, zero, 1.0)
            for s in (1.0, 100.0)]
    assert float(outs[0][0]) == float(outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # T_j = R for every j: the priority is |R - q|
    q = th[torch.arange(B), act].mean(-1)
    torch.testing.assert_close(outs[0][1], (R - q).abs(), rtol=0, atol=1e-15)


# ----------------------------------------------------------------------- model
def test_model_keys_shapes_and_mean():
    A, N = 6, 32
    torch.manual_seed(0)
    net = DuellingDQN((4, 84, 84), A, num_atoms=N, dist_head="quantile")
    c51 = DuellingDQN((4, 84, 84), A, num_atoms=N)
    sd, sc = net.state_dict(), c51.state_dict()
    assert tuple(sd.keys()) == REFERENCE_KEYS == tuple(sc.keys())
    assert {k: v.shape for k, v in sd.items()} == {k: v.shape for k, v in sc.items()}
    assert sd["value.weight"].shape == (N, 512) and sd["advantage.weight"].shape == (A * N, 512)
    assert not hasattr(net, "support") and hasattr(c51, "support")
    x = torch.randint(0, 255, (3, 4, 84, 84), dtype=torch.uint8)
    with torch.no_grad():
        v, a, q = net(x)
        th = net.quantiles(x)
    assert v.shape == (3, N) and a.shape == (3, A * N) and q.shape == (3, A) and th.shape == (3, A, N)
    torch.testing.assert_close(q, th.mean(-1), rtol=0, atol=0)
    # advantage row a N + i is action a, quantile i; the dueling mean is taken per quantile
    adv = a.reshape(3, A, N)
    torch.testing.assert_close(th, v[:, None] + adv - adv.mean(1, keepdim=True), rtol=0, atol=0)
    mlp = build_network("mlp", [4], 2, num_atoms=11, dist_head="quantile")
    assert mlp.quantiles(torch.randn(5, 4)).shape == (5, 2, 11)
    with pytest.raises(ValueError, match="dist_head"):
        DuellingDQN((4, 84, 84), A, num_atoms=N, dist_head="iqn")


def test_flat_round_trip_is_exact():
    A, N = 6, 32
    torch.manual_seed(1)
    net = DuellingDQN((4, 84, 84), A, num_atoms=N, dist_head="quantile")
    lay = FlatLayout(nature_segments(4, A, 64, N))
    flat = torch.zeros(lay.numel)
    reference_state_to_flat(net.state_dict(), lay.views(flat))
    back = flat_to_reference_state(lay.views(flat), 64)
    assert tuple(back.keys()) == REFERENCE_KEYS
    for k, t in net.state_dict().items():
        assert torch.equal(back[k], t), k


# ----------------------------------------------------- fused backward vs autograd
def _setup(N, A=6, network="nature64", **rt):
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": 8},
                                "Runtime": {"grad_clip": 40.0, "network": network, "presample": False,
                                            "num_atoms": N, "dist_head": "quantile", **rt}})
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


@pytest.mark.parametrize("N", [7, 32])
def test_fused_backward_matches_autograd(N):
    cfg, rp = _setup(N)
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.N == N and L.quantile and L.dhead.shape == (8, 7 * N) and not L._defer_fc_epilogue
    T = TorchLearner(cfg, "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    L._seg1()
    L._seg2()
    B, S = L.B, L.S
    batch = dict(S_t=L.frames[:B], S_tpn=L.frames[B:2 * B], A_t=S["act"], R=S["rew"], Gamma=S["gam"],
                 weights=S["weights"])
    lref, td = T.compute_loss_and_priorities(batch)
    T.optimizer.zero_grad()
    lref.backward()
    assert abs(float(lref) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref)))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    for k, p in T.Q.named_parameters():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7)
    assert float(gf["value.weight"].norm()) > 0 and float(gf["advantage.weight"].norm()) > 0
    with torch.no_grad():
        torch.testing.assert_close(L.q_values(L.frames[:B]), T.Q(L.frames[:B])[2], rtol=1e-5, atol=1e-5)


def test_fused_step_updates_params_and_priorities():
    cfg, rp = _setup(32)
    L = FusedNatureLearner(cfg, "cpu", rp)
    p0, leaf0 = L.p32.clone(), rp.leaf.clone()
    L.step()
    o = L.layout.offsets
    assert not torch.equal(p0[o["wv"]:o["wfc"]], L.p32[o["wv"]:o["wfc"]])      # the heads moved
    idx = L.S["idx"]
    assert not torch.equal(leaf0[idx], rp.leaf[idx])
    assert torch.isfinite(rp.leaf).all() and L.num_q_updates == 1


# ---------------------------------------------------------------------- config
def _cfg(**rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": rt})


@pytest.mark.parametrize("rt,key", [
    (dict(dist_head="quantile"), "dist_head"),                        # num_atoms = 1
    (dict(num_atoms=1, dist_head="quantile"), "dist_head"),
    (dict(num_atoms=32, dist_head="iqn"), "dist_head"),
    (dict(num_atoms=32, dist_head="quantile", huber_delta=0.0), "huber_delta"),
    (dict(num_atoms=32, dist_head="quantile", huber_delta=-1.0), "huber_delta"),
    (dict(num_atoms=32, dist_head="quantile", network="impala"), "num_atoms"),
    (dict(num_atoms=32, dist_head="quantile", force_dp=True), "num_atoms"),
    (dict(num_atoms=32, dist_head="quantile", world_size=2), "num_atoms"),
])
def test_config_refusals(rt, key):
    with pytest.raises(ValueError, match=key):
        _cfg(**rt)


def test_config_accepts_and_round_trips():
    c = _cfg()
    assert c.Runtime.dist_head == "categorical" and c.Runtime.num_atoms == 1 and not c.quantile
    assert _cfg(num_atoms=51).head_kw()["dist_head"] == "categorical" and not _cfg(num_atoms=51).quantile
    assert _cfg(num_atoms=51, huber_delta=0.0).distributional        # kappa is the quantile head's only
    q = _cfg(num_atoms=32, dist_head="quantile", huber_delta=0.5, v_min=-1.0, v_max=1.0)
    assert q.quantile and q.distributional and q.head_kw()["dist_head"] == "quantile"
    c2 = ApexConfig.from_dict(q.to_dict())
    assert c2.to_dict() == q.to_dict()
    assert (c2.Runtime.num_atoms, c2.Runtime.dist_head, c2.Runtime.huber_delta) == (32, "quantile", 0.5)
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "pong_1gpu_qr.json")
    f = ApexConfig.load(path)
    assert f.quantile and f.Runtime.num_atoms == 32 and f.network == "nature64"


def test_learners_without_a_distributional_head_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    cfg, rp = _setup(32)
    with pytest.raises(ValueError, match="num_atoms"):
        GraphLearner(cfg, "cpu", rp)

    class Comm:                      # a second rank: the data-parallel step
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="num_atoms"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_and_kind_mismatch(tmp_path):
    cfg, rp = _setup(32)
    L = FusedNatureLearner(cfg, "cpu", rp)
    L.step()
    L.step()
    path = str(tmp_path / "qr.pt")
    L.save(path)
    cfg2, rp2 = _setup(32)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    assert not torch.equal(L.p32, L2.p32)
    assert L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.pbf, L2.pbf)):
        assert torch.equal(a, b)
    assert L2.num_q_updates == 2
    # the categorical head at the same N: same shapes, another meaning
    cfg3, rp3 = _setup(32, dist_head="categorical")
    L3 = FusedNatureLearner(cfg3, "cpu", rp3)
    p3 = L3.p32.clone()
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        L3.load(path)
    assert torch.equal(p3, L3.p32)                                 # nothing was copied
    path3 = str(tmp_path / "c51.pt")
    L3.save(path3)
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        L2.load(path3)
    # another quantile count is the shape mismatch it always was
    cfg4, rp4 = _setup(21)
    with pytest.raises(ValueError, match="Runtime.num_atoms"):
        FusedNatureLearner(cfg4, "cpu", rp4).load(path)
    # a reference-format state dict carries no config: only its shapes are judged
    L2.load_reference_state_dict(DuellingDQN((4, 84, 84), 6, num_atoms=32).state_dict())
    # the torch learner refuses the other kind too
    mk = lambda kind: ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},   # noqa: E731
                                            "Runtime": {"num_atoms": 11, "dist_head": kind}})
    Tq, Tc = TorchLearner(mk("quantile"), "cpu"), TorchLearner(mk("categorical"), "cpu")
    pq = str(tmp_path / "mlp_qr.pt")
    Tq.save(pq)
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        Tc.load(pq)
    assert TorchLearner(mk("quantile"), "cpu").load(pq)


# --------------------------------------------------------------- torch learner
def test_mlp_torch_learner_trains_on_a_fixed_batch():
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 1000},
                                "Runtime": {"num_atoms": 11, "dist_head": "quantile", "lr": 1e-3}})
    T = TorchLearner(cfg, "cpu")
    g = torch.Generator().manual_seed(3)
    B = 32
    batch = dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                 A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g) * 3,
                 Gamma=torch.full((B,), 0.97), weights=torch.rand(B, generator=g) + 0.5)
    first = T.step(batch)
    assert first["td_abs"].shape == (B,) and np.isfinite(first["td_abs"]).all()
    for _ in range(48):
        T.step(batch)
    last = T.step(batch)
    assert T.num_q_updates == 50
    assert last["loss"] < first["loss"]
    # the loss is the weighted quantile Huber loss of learner/losses.py on this batch
    with torch.no_grad():
        ref, _ = quantile_huber_loss(T.Q.quantiles(batch["S_t"]), T.Q(batch["S_tpn"])[2],
                                     T.Q_target.quantiles(batch["S_tpn"]), batch["A_t"], batch["R"], batch["Gamma"],
                                     1.0, batch["weights"])
        now, _ = T.compute_loss_and_priorities(batch)
    assert float(ref) == float(now)
