"""Implicit quantile (IQN) head through the layers above the kernels, without a GPU: the modules'
``quantiles_at``, the flat layout and checkpoints, the config, the fused learner's backward on the
torch backend against autograd, the MLP torch learner and a short inline CartPole run."""
import math
import os

import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import iqn
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.dueling import REFERENCE_KEYS, DuellingDQN, build_network
from apex_dqn_amd.models.flat_params import (FlatLayout, flat_to_reference_state, nature_segments,
                                             reference_state_to_flat)
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- module
def test_quantiles_at_follows_the_definition_on_a_hand_built_module():
    """hidden = 2, A = 2: every weight set by hand, theta written out from the issue's formulas."""
    from apex_dqn_amd.models.dueling import MLPDuellingDQN
    net = MLPDuellingDQN([1], 2, hidden=2, num_atoms=3, dist_head="implicit", iqn_actor_samples=4)
    assert net.value.weight.shape == (1, 2) and net.advantage.weight.shape == (2, 2)       # the scalar head's shapes
    assert net.tau_embed.weight.shape == (4, 64) and net.tau_embed.bias.shape == (4,)
    with torch.no_grad():
        net.layer1[0].weight.fill_(1.0), net.layer1[0].bias.zero_()
        net.value_stream_layer[0].weight.copy_(torch.tensor([[1.0, 0.0], [0.0, 2.0]]))
        net.value_stream_layer[0].bias.zero_()
        net.advantage_stream_layer[0].weight.copy_(torch.tensor([[0.5, 0.0], [0.0, 1.0]]))
        net.advantage_stream_layer[0].bias.zero_()
        net.tau_embed.weight.zero_()
        net.tau_embed.weight[:, 0] = torch.tensor([1.0, 2.0, -1.0, 0.5])       # on c_0 = 1
        net.tau_embed.weight[:, 1] = torch.tensor([1.0, 0.0, 3.0, 0.0])        # on c_1 = cos(pi tau)
        net.tau_embed.bias.copy_(torch.tensor([0.0, 0.5, 0.0, -1.0]))
        net.value.weight.copy_(torch.tensor([[1.0, -1.0]])), net.value.bias.fill_(0.25)
        net.advantage.weight.copy_(torch.tensor([[1.0, 1.0], [2.0, 0.0]])), net.advantage.bias.copy_(torch.tensor([0.0, 1.0]))
    x = torch.tensor([[3.0]])
    tau = torch.tensor([[0.0, 0.5, 1.0]])
    th = net.quantiles_at(x, tau)
    assert th.shape == (1, 2, 3)
    hv, ha = (3.0, 6.0), (1.5, 3.0)                      # relu(W * 3) of the two streams
    want = []
    for t in (0.0, 0.5, 1.0):
        c1 = math.cos(math.pi * t)
        pre = (1.0 + c1, 2.5, -1.0 + 3.0 * c1, -0.5)
        phi = [max(p, 0.0) for p in pre]
        xv, xa = (hv[0] * phi[0], hv[1] * phi[1]), (ha[0] * phi[2], ha[1] * phi[3])
        v = xv[0] - xv[1] + 0.25
        adv = (xa[0] + xa[1], 2.0 * xa[0] + 1.0)
        m = 0.5 * (adv[0] + adv[1])
        want.append((v + adv[0] - m, v + adv[1] - m))
    torch.testing.assert_close(th[0], torch.tensor(want).t().contiguous(), rtol=1e-6, atol=1e-6)
    # forward: q = the mean over the K midpoints
    mid = iqn.midpoint_taus(4)[None, :]
    torch.testing.assert_close(net(x)[2], net.quantiles_at(x, mid).mean(-1), rtol=0, atol=0)
    assert build_network("nature64", [4, 84, 84], 3, num_atoms=5, dist_head="implicit").quantiles_at(
        torch.zeros(2, 4, 84, 84, dtype=torch.uint8), torch.rand(2, 7)).shape == (2, 3, 7)
    with pytest.raises(ValueError, match="noisy"):
        DuellingDQN((4, 84, 84), 3, num_atoms=5, dist_head="implicit", noisy=True)


def test_flat_layout_keeps_every_offset_and_round_trips_tau_embed():
    A = 6
    torch.manual_seed(1)
    net = DuellingDQN((4, 84, 84), A, num_atoms=8, dist_head="implicit")
    lay, scalar = FlatLayout(nature_segments(4, A, 64, 1, implicit=True)), FlatLayout(nature_segments(4, A, 64, 1))
    assert all(lay.offsets[k] == o and lay.shapes[k] == scalar.shapes[k] for k, o in scalar.offsets.items())
    assert lay.offsets["wtau"] >= scalar.offsets["bfc"] + 1024 and lay.offsets["btau"] == lay.offsets["wtau"] + 1024 * 64
    assert lay.shapes["wtau"] == (1024, 64) and lay.shapes["btau"] == (1024,) and lay.offsets["wtau"] % 64 == 0
    flat = torch.zeros(lay.numel)
    reference_state_to_flat(net.state_dict(), lay.views(flat))
    back = flat_to_reference_state(lay.views(flat), 64)
    assert tuple(back.keys()) == REFERENCE_KEYS + ("tau_embed.weight", "tau_embed.bias")
    for k, t in net.state_dict().items():
        assert torch.equal(back[k], t), k
    # a state of the other kind is refused before anything is copied, both ways
    f0 = torch.zeros(scalar.numel)
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        reference_state_to_flat(net.state_dict(), scalar.views(f0))
    assert not f0.any()
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        reference_state_to_flat(DuellingDQN((4, 84, 84), A).state_dict(), lay.views(torch.zeros(lay.numel)))


# ---------------------------------------------------------------------- config
def _cfg(**rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": rt})


@pytest.mark.parametrize("rt,key", [
    (dict(dist_head="implicit"), "dist_head"),                        # num_atoms = 1
    (dict(num_atoms=8, dist_head="implicit", huber_delta=0.0), "huber_delta"),
    (dict(num_atoms=8, dist_head="implicit", iqn_actor_samples=0), "iqn_actor_samples"),
    (dict(num_atoms=8, dist_head="implicit", iqn_actor_samples=65), "iqn_actor_samples"),
    (dict(num_atoms=8, dist_head="implicit", network="impala"), "num_atoms"),
    (dict(num_atoms=8, dist_head="implicit", force_dp=True), "num_atoms"),
    (dict(num_atoms=8, dist_head="implicit", world_size=2), "num_atoms"),
    (dict(num_atoms=8, dist_head="implicit", noisy=True), "Runtime.noisy"),
    (dict(num_atoms=8, dist_head="implicit", munchausen=True), "Runtime.munchausen"),
])
def test_config_refusals(rt, key):
    with pytest.raises(ValueError, match=key):
        _cfg(**rt)


def test_config_accepts_and_round_trips():
    c = _cfg(num_atoms=8, dist_head="implicit")
    assert c.implicit and c.distributional and not c.quantile and c.Runtime.iqn_actor_samples == 32
    assert c.head_kw()["iqn_actor_samples"] == 32 and "iqn_actor_samples" not in _cfg(num_atoms=8).head_kw()
    assert not _cfg().implicit and not _cfg(num_atoms=8, dist_head="quantile").implicit
    assert ApexConfig.from_dict(c.to_dict()).to_dict() == c.to_dict()
    f = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_iqn.json"))
    assert f.implicit and f.Runtime.num_atoms == 8 and f.Runtime.iqn_actor_samples == 32 and f.network == "nature64"


# ------------------------------------------------- fused learner (torch backend)
def _setup(N, A=4, **rt):
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": 8},
                                "Runtime": {"grad_clip": 40.0, "presample": False, "num_atoms": N,
                                            "dist_head": "implicit", **rt}})
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


@pytest.mark.parametrize("A,N", [(4, 8), (3, 5)])
def test_fused_backward_matches_autograd(A, N):
    """Every gradient segment (the embedding's included) of the fused step on the torch backend against
    autograd through the torch learner, which draws the same fractions (the same update index)."""
    cfg, rp = _setup(N, A)
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.implicit and L.N == N and L.Nh == 1 and L.dhead.shape == (8, (A + 1) * N) and not L._defer_fc_epilogue
    assert L.P["wv"].shape == (512,) and L.P["wa"].shape == (A, 512) and L.P["wtau"].shape == (1024, 64)
    T = TorchLearner(cfg, "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    L._seg1()
    L._seg2()
    B, S = L.B, L.S
    batch = dict(S_t=L.frames[:B], S_tpn=L.frames[B:2 * B], A_t=S["act"], R=S["rew"], Gamma=S["gam"],
                 weights=S["weights"])
    lref, td = T.compute_loss_and_priorities(batch)
    assert torch.equal(T.last_taus, L.tau_out) and torch.equal(L.tau_out, iqn.learner_taus(iqn.iqn_seed(cfg.Runtime.seed), 0, B, N))
    T.optimizer.zero_grad()
    lref.backward()
    assert abs(float(lref.detach()) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref.detach())))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    for k, p in T.Q.named_parameters():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7)
    assert float(gf["tau_embed.weight"].norm()) > 0 and float(gf["tau_embed.bias"].norm()) > 0
    with torch.no_grad():
        torch.testing.assert_close(L.q_values(L.frames[:B]), T.Q(L.frames[:B])[2], rtol=1e-5, atol=1e-5)


def test_consecutive_updates_draw_different_taus_and_move_the_embedding():
    cfg, rp = _setup(8)
    L = FusedNatureLearner(cfg, "cpu", rp)
    p0, leaf0 = L.p32.clone(), rp.leaf.clone()
    L.step()
    t0 = L.tau_out.clone()
    L.step()
    assert not torch.equal(t0, L.tau_out)
    sq = iqn.iqn_seed(cfg.Runtime.seed)
    assert torch.equal(t0, iqn.learner_taus(sq, 0, L.B, 8)) and torch.equal(L.tau_out, iqn.learner_taus(sq, 1, L.B, 8))
    o = L.layout.offsets
    assert not torch.equal(p0[o["wtau"]:], L.p32[o["wtau"]:]) and not torch.equal(p0[o["wv"]:o["wfc"]], L.p32[o["wv"]:o["wfc"]])
    assert not torch.equal(leaf0[L.S["idx"]], rp.leaf[L.S["idx"]]) and L.num_q_updates == 2 and L.update_index() == 2


def test_learners_without_the_head_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    cfg, rp = _setup(8)
    with pytest.raises(ValueError, match="num_atoms"):
        GraphLearner(cfg, "cpu", rp)

    class Comm:                      # a second rank: the data-parallel step
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="num_atoms"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_and_kind_mismatch(tmp_path):
    cfg, rp = _setup(8)
    L = FusedNatureLearner(cfg, "cpu", rp)
    L.step()
    L.step()
    path = str(tmp_path / "iqn.pt")
    L.save(path)
    cfg2, rp2 = _setup(8)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    assert not torch.equal(L.p32, L2.p32)
    assert L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.pbf, L2.pbf)):
        assert torch.equal(a, b)
    assert L2.num_q_updates == 2 and L2.update_index() == 2
    # the resumed learner draws update 2's fractions, as the first one does
    L.step(), L2.step()
    assert torch.equal(L.tau_out, L2.tau_out) and torch.equal(L.tau_out, iqn.learner_taus(iqn.iqn_seed(cfg.Runtime.seed), 2, 8, 8))
    # the quantile head at the same N, and the scalar head, refuse it and are refused, naming the key
    for other in (dict(num_atoms=8, dist_head="quantile"), dict(num_atoms=1, dist_head="categorical")):
        cfg3, rp3 = _setup(8)
        cfg3 = ApexConfig.from_dict({**cfg3.to_dict(), "Runtime": {**cfg3.to_dict()["Runtime"], **other}})
        L3 = FusedNatureLearner(cfg3, "cpu", rp3)
        p3 = L3.p32.clone()
        with pytest.raises(ValueError, match="Runtime.dist_head"):
            L3.load(path)
        assert torch.equal(p3, L3.p32)                                 # nothing was copied
        path3 = str(tmp_path / "other.pt")
        L3.save(path3)
        p2 = L2.p32.clone()
        with pytest.raises(ValueError, match="Runtime.dist_head"):
            L2.load(path3)
        assert torch.equal(p2, L2.p32)
    # the torch learner refuses the other kind too
    mk = lambda kind: ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},   # noqa: E731
                                            "Runtime": {"num_atoms": 8, "dist_head": kind}})
    Ti, Tq = TorchLearner(mk("implicit"), "cpu"), TorchLearner(mk("quantile"), "cpu")
    pi, pq = str(tmp_path / "mlp_iqn.pt"), str(tmp_path / "mlp_qr.pt")
    Ti.save(pi), Tq.save(pq)
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        Tq.load(pi)
    with pytest.raises(ValueError, match="Runtime.dist_head"):
        Ti.load(pq)
    assert TorchLearner(mk("implicit"), "cpu").load(pi)


# --------------------------------------------------------------- torch learner
def test_mlp_torch_learner_trains_on_a_fixed_batch():
    from apex_dqn_amd.learner.losses import iqn_loss
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 1000},
                                "Runtime": {"num_atoms": 8, "dist_head": "implicit", "lr": 1e-3}})
    T = TorchLearner(cfg, "cpu")
    g = torch.Generator().manual_seed(3)
    B = 32
    batch = dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                 A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g) * 3,
                 Gamma=torch.full((B,), 0.97), weights=torch.rand(B, generator=g) + 0.5)
    first = T.step(batch)
    assert first["td_abs"].shape == (B,) and np.isfinite(first["td_abs"]).all()
    losses = [T.step(batch)["loss"] for _ in range(98)]
    assert T.num_q_updates == 99
    assert np.mean(losses[-10:]) < np.mean([first["loss"]] + losses[:9])     # (the draws change: means of ten)
    # the loss is iqn_loss of learner/losses.py at this update's fractions
    with torch.no_grad():
        now, _ = T.compute_loss_and_priorities(batch)
        t = iqn.learner_taus(iqn.iqn_seed(cfg.Runtime.seed), 99, B, 8)
        ref, _ = iqn_loss(T.Q.quantiles_at(batch["S_t"], t[:, 0]), t[:, 0], T.Q.quantiles_at(batch["S_tpn"], t[:, 1]).mean(-1),
                          T.Q_target.quantiles_at(batch["S_tpn"], t[:, 2]), batch["A_t"], batch["R"], batch["Gamma"],
                          1.0, batch["weights"])
    assert float(ref) == float(now)


def test_inline_cartpole_runs_with_the_head():
    from apex_dqn_amd.runtime.loops import train_inline
    cfg = ApexConfig.load(os.path.join(ROOT, "configs", "cartpole.json"),
                          ["Runtime.num_atoms=8", "Runtime.dist_head=implicit", "Runtime.iqn_actor_samples=4"])
    assert cfg.implicit and cfg.network == "mlp"
    out = train_inline(cfg, 30)
    T = out["learner"]
    assert T.num_q_updates == 30 and len(out["losses"]) == 30 and np.isfinite(out["losses"]).all()
    assert T.Q.iqn_actor_samples == 4 and T.Q.iqn_draw is None         # the learner's own forward: the midpoints


def test_cpu_actor_groups_draw_the_gpu_groups_fractions():
    """The hook of the inline loop and the actor processes: call t of group g uses stream_taus(seed_q, 64 t +
    actor_stream(g)), K per env row -- what ``iqn_actor_head_kernel`` draws -- and the q is their mean."""
    from apex_dqn_amd.learner.noisy import actor_stream
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Runtime": {"num_atoms": 8, "dist_head": "implicit", "iqn_actor_samples": 5}})
    net = build_network(cfg.network, [4], 2, **cfg.head_kw())
    hook = iqn.actor_tau_hook(cfg, net, 3)
    x = torch.randn(6, 4)
    q_mid = net(x)[2]
    qs = []
    for t in (0, 1):
        hook(t)
        tau = iqn.stream_taus(iqn.iqn_seed(cfg.Runtime.seed), 64 * t + actor_stream(3), 6, 5)
        assert torch.equal(tau, iqn.actor_taus(iqn.iqn_seed(cfg.Runtime.seed), t, 3, 6, 5))
        q = net(x)[2]
        torch.testing.assert_close(q, net.quantiles_at(x, tau).mean(-1), rtol=0, atol=0)
        qs.append(q)
    assert not torch.equal(qs[0], qs[1]) and not torch.equal(qs[0], q_mid)
    assert iqn.actor_tau_hook(ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2,
                                                                 "name": "CartPole-v1"}}), net, 0) is None
