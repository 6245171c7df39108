"""Distributional (C51) dueling head on the CPU: the projection by hand, the module and
flat layout, the fused learner's hand-written backward against autograd, the config
refusals, checkpoints, and the torch learner training on a fixed batch."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.losses import c51_loss, c51_project
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.dueling import REFERENCE_KEYS, DuellingDQN, build_network, c51_support
from apex_dqn_amd.models.flat_params import (FlatLayout, flat_to_reference_state, nature_segments,
                                             reference_state_to_flat)
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard


# ------------------------------------------------------------------ projection
def _proj(p, R, G):
    return c51_project(torch.tensor([p], dtype=torch.float64), torch.tensor([R], dtype=torch.float64),
                       torch.tensor([G], dtype=torch.float64), -2.0, 2.0)[0]


def test_projection_by_hand():
    p = [0.1, 0.2, 0.3, 0.25, 0.15]
    torch.testing.assert_close(_proj(p, 0.5, 0.0), torch.tensor([0, 0, .5, .5, 0], dtype=torch.float64),
                               rtol=0, atol=1e-15)
    torch.testing.assert_close(_proj(p, 7.0, 0.0), torch.tensor([0, 0, 0, 0, 1.], dtype=torch.float64),
                               rtol=0, atol=1e-15)
    torch.testing.assert_close(_proj(p, -7.0, 0.9), torch.tensor([1., 0, 0, 0, 0], dtype=torch.float64),
                               rtol=0, atol=1e-15)


def test_projection_keeps_mass_and_mean_when_nothing_clamps():
    g = torch.Generator().manual_seed(0)
    B, N = 16, 5
    p = torch.softmax(torch.randn(B, N, generator=g, dtype=torch.float64), -1)
    R = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 0.3      # |R| + 0.9 * 2 < 2
    G = torch.full((B,), 0.9, dtype=torch.float64)
    m = c51_project(p, R, G, -2.0, 2.0)
    z = c51_support(N, -2.0, 2.0, torch.float64)
    assert float((m.sum(-1) - 1).abs().max()) < 1e-12
    assert float(((m * z).sum(-1) - (R + G * (p * z).sum(-1))).abs().max()) < 1e-12
    assert float(m.min()) >= 0.0


# ----------------------------------------------------------------------- model
def test_model_keys_shapes_and_expectation():
    A, N = 6, 51
    net = DuellingDQN((4, 84, 84), A, num_atoms=N, v_min=-10.0, v_max=10.0)
    sd = net.state_dict()
    assert tuple(sd.keys()) == REFERENCE_KEYS
    assert sd["value.weight"].shape == (N, 512) and sd["value.bias"].shape == (N,)
    assert sd["advantage.weight"].shape == (A * N, 512) and sd["advantage.bias"].shape == (A * N,)
    x = torch.randint(0, 255, (3, 4, 84, 84), dtype=torch.uint8)
    with torch.no_grad():
        v, a, q = net(x)
        lp = net.log_probs(x)
    assert v.shape == (3, N) and a.shape == (3, A * N) and q.shape == (3, A) and lp.shape == (3, A, N)
    z = c51_support(N, -10.0, 10.0)
    torch.testing.assert_close(q, (lp.exp() * z).sum(-1), rtol=0, atol=0)
    torch.testing.assert_close(lp.exp().sum(-1), torch.ones(3, A), rtol=1e-6, atol=1e-6)
    # advantage row a N + i is action a, atom i; the dueling mean is taken per atom
    adv = a.reshape(3, A, N)
    ref = torch.log_softmax(v[:, None] + adv - adv.mean(1, keepdim=True), -1)
    torch.testing.assert_close(lp, ref, rtol=0, atol=0)
    mlp = build_network("mlp", [4], 2, num_atoms=11, v_min=0.0, v_max=5.0)
    assert mlp.log_probs(torch.randn(5, 4)).shape == (5, 2, 11)
    with pytest.raises(ValueError, match="num_atoms"):
        build_network("impala", [4, 84, 84], 4, num_atoms=51)


@pytest.mark.parametrize("c1", [64, 32])
def test_flat_round_trip_is_exact(c1):
    A, N = 6, 51
    torch.manual_seed(1)
    net = DuellingDQN((4, 84, 84), A, conv1_channels=c1, num_atoms=N)
    lay = FlatLayout(nature_segments(4, A, 64, N))
    assert lay.shapes["wv"] == (N, 512) and lay.shapes["bv"] == (N,)
    assert lay.shapes["wa"] == (A * N, 512) and lay.shapes["ba"] == (A * N,)
    flat = torch.zeros(lay.numel)
    reference_state_to_flat(net.state_dict(), lay.views(flat))
    back = flat_to_reference_state(lay.views(flat), c1)
    assert tuple(back.keys()) == REFERENCE_KEYS
    for k, t in net.state_dict().items():
        assert torch.equal(back[k], t), k


def test_num_atoms_1_keeps_the_scalar_layout():
    a, b = FlatLayout(nature_segments(4, 6, 64)), FlatLayout(nature_segments(4, 6, 64, 1))
    assert a.numel == b.numel and a.shapes == b.shapes and a.offsets == b.offsets
    assert a.shapes["wv"] == (512,) and a.shapes["bv"] == (1,) and a.shapes["wa"] == (6, 512)


# ----------------------------------------------------- fused backward vs autograd
def _setup(N, A=6, network="nature64", **rt):
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": 8},
                                "Runtime": {"grad_clip": 40.0, "network": network, "presample": False,
                                            "num_atoms": N, "v_min": -10.0, "v_max": 10.0, **rt}})
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


@pytest.mark.parametrize("N", [7, 51])
def test_fused_backward_matches_autograd(N):
    cfg, rp = _setup(N)
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.N == N and L.dhead.shape == (8, 7 * N) and not L._defer_fc_epilogue
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
    with torch.no_grad():
        torch.testing.assert_close(L.q_values(L.frames[:B]), T.Q(L.frames[:B])[2], rtol=1e-5, atol=1e-5)


def test_fused_step_updates_params_and_priorities():
    cfg, rp = _setup(51)
    L = FusedNatureLearner(cfg, "cpu", rp)
    p0, leaf0, ctr0 = L.p32.clone(), rp.leaf.clone(), int(rp.ctr[0])
    L.step()
    assert not torch.equal(p0, L.p32)
    o = L.layout.offsets
    assert not torch.equal(p0[o["wv"]:o["wfc"]], L.p32[o["wv"]:o["wfc"]])      # the heads moved too
    idx = L.S["idx"]
    assert not torch.equal(leaf0[idx], rp.leaf[idx])
    assert torch.isfinite(rp.leaf).all() and L.num_q_updates == 1
    assert int(rp.ctr[0]) - ctr0 == 1         # the priority write-back bumps the draw counter once


# ---------------------------------------------------------------------- config
def _cfg(**rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": rt})


@pytest.mark.parametrize("rt,key", [
    (dict(num_atoms=0), "num_atoms"), (dict(num_atoms=65), "num_atoms"), (dict(num_atoms=-3), "num_atoms"),
    (dict(num_atoms=2.5), "num_atoms"),
    (dict(num_atoms=51, v_min=3.0, v_max=3.0), "v_min"), (dict(v_min=1.0, v_max=-1.0), "v_min"),
    (dict(num_atoms=51, network="impala"), "num_atoms"),
    (dict(num_atoms=51, world_size=2), "num_atoms"),
    (dict(num_atoms=51, force_dp=True), "num_atoms"),
])
def test_config_refusals(rt, key):
    with pytest.raises(ValueError, match=key):
        _cfg(**rt)


def test_config_accepts_and_round_trips():
    for n in (1, 2, 51, 64):
        c = _cfg(num_atoms=n)
        assert c.Runtime.num_atoms == n and c.distributional == (n >= 2)
    c = ApexConfig.from_dict(_cfg(num_atoms=51, v_min=-5.0, v_max=20.0).to_dict())
    assert (c.Runtime.num_atoms, c.Runtime.v_min, c.Runtime.v_max) == (51, -5.0, 20.0)
    assert _cfg().Runtime.num_atoms == 1
    mlp = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Runtime": {"num_atoms": 11}})
    assert mlp.network == "mlp" and mlp.distributional


def test_learners_without_a_distributional_head_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    cfg, rp = _setup(51)
    with pytest.raises(ValueError, match="num_atoms"):
        GraphLearner(cfg, "cpu", rp)

    class Comm:                      # a second rank: the data-parallel step
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="num_atoms"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_and_mismatch(tmp_path):
    cfg, rp = _setup(51)
    L = FusedNatureLearner(cfg, "cpu", rp)
    L.step()
    L.step()
    path = str(tmp_path / "c51.pt")
    L.save(path)
    cfg2, rp2 = _setup(51)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    assert not torch.equal(L.p32, L2.p32)
    assert L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.pbf, L2.pbf)):
        assert torch.equal(a, b)
    assert L2.num_q_updates == 2
    for n in (1, 21):
        cfg3, rp3 = _setup(n)
        L3 = FusedNatureLearner(cfg3, "cpu", rp3)
        p3 = L3.p32.clone()
        with pytest.raises(ValueError, match="Runtime.num_atoms"):
            L3.load(path)
        o = L3.layout.offsets
        assert torch.equal(p3[o["wv"]:], L3.p32[o["wv"]:])       # nothing copied misaligned into the heads
    with pytest.raises(ValueError, match="Runtime.num_atoms"):
        L.load_reference_state_dict(DuellingDQN((4, 84, 84), 6).state_dict())


# --------------------------------------------------------------- torch learner
def test_mlp_torch_learner_trains_on_a_fixed_batch():
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 1000},
                                "Runtime": {"num_atoms": 11, "v_min": 0.0, "v_max": 10.0, "lr": 1e-3}})
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
    # the loss is the weighted cross-entropy of learner/losses.py on this batch
    with torch.no_grad():
        ref, _ = c51_loss(T.Q.log_probs(batch["S_t"]), T.Q(batch["S_tpn"])[2],
                          T.Q_target.log_probs(batch["S_tpn"]).exp(), batch["A_t"], batch["R"], batch["Gamma"],
                          0.0, 10.0, batch["weights"])
        now, _ = T.compute_loss_and_priorities(batch)
    assert float(ref) == float(now)
