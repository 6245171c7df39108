"""Factorised NoisyNet fc and head layers on the CPU: the noise draw's host mirror, the
``NoisyLinear`` module by hand, the flat layout, the fused learner's hand-written backward
(with the sigma gradients) against autograd for every head kind, the noise schedule over
updates, the config refusals, checkpoints, and the torch learner on the MLP."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import noisy as NZ
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.dueling import (NOISY_LAYERS, REFERENCE_KEYS, SIGMA_KEYS, DuellingDQN, MLPDuellingDQN,
                                         NoisyLinear, build_network)
from apex_dqn_amd.models.flat_params import (FlatLayout, flat_to_reference_state, nature_segments,
                                             reference_state_to_flat)
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

SEED = NZ.noise_seed(0)


# ---------------------------------------------------------------------- mirror
@pytest.mark.parametrize("A,N", [(4, 1), (3, 7)])
def test_noise_vectors_lengths_and_order(A, N):
    v = NZ.noise_vectors(SEED, 5, 0, A, N)
    want = [("fc_in_v", 3136), ("fc_in_a", 3136), ("fc_out", 1024), ("v_in", 512), ("a_in", 512), ("v_out", N),
            ("a_out", A * N)]
    assert [(k, v[k].numel()) for k, _ in want] == want
    K = sum(n for _, n in want)
    assert v["xi"].numel() == K == NZ.xi_offsets(A, N)["K"]
    assert torch.equal(torch.cat([v[k] for k, _ in want]), v["xi"]) and v["xi"].dtype == torch.float64
    # index k of the concatenation keys the draw: a longer head keeps the shared prefix
    w = NZ.noise_vectors(SEED, 5, 0, A + 1, N)
    assert torch.equal(w["xi"][:K], v["xi"])


def test_noise_is_deterministic_and_keyed_by_seed_u_s():
    a = NZ.noise_vectors(SEED, 3, 1, 4, 1)["xi"]
    assert torch.equal(a, NZ.noise_vectors(SEED, 3, 1, 4, 1)["xi"])
    for other in ((SEED, 4, 1), (SEED, 3, 0), (SEED, 3, 2), (NZ.noise_seed(1), 3, 1)):
        b = NZ.noise_vectors(other[0], other[1], other[2], 4, 1)["xi"]
        assert not torch.equal(a, b) and float((a - b).abs().max()) > 0.5
    # (u, s) and (u', s') never share a counter word: c = 64 u + s, s < 64
    assert NZ.STREAMS_PER_INDEX == 64 and NZ.actor_stream(0) == 2 and NZ.actor_stream(61) == 63
    assert NZ.noise_seed(0) != 0 and NZ.noise_seed(0) != NZ.noise_seed(1)


def test_gaussian_moments_and_xi_transform():
    n = 200_000
    g = NZ.gaussians(SEED, 0, 0, n)
    assert abs(g.mean()) < 4 / np.sqrt(n), g.mean()
    assert abs(g.var() - 1) < 4 * np.sqrt(2 / n), g.var()
    xi = NZ.xi_of(g)
    assert np.array_equal(xi, np.sign(g) * np.sqrt(np.abs(g)))
    K = NZ.xi_offsets(4, 1)["K"]
    assert np.array_equal(NZ.noise_vectors(SEED, 0, 0, 4, 1)["xi"].numpy(), xi[:K])


# ----------------------------------------------------------------- NoisyLinear
def test_noisy_linear_by_hand():
    lin = NoisyLinear(3, 2, sigma0=0.5)
    with torch.no_grad():
        lin.weight.copy_(torch.tensor([[1., 2., 3.], [4., 5., 6.]]))
        lin.bias.copy_(torch.tensor([0.5, -0.5]))
        lin.weight_sigma.copy_(torch.tensor([[.1, .2, .3], [.4, .5, .6]]))
        lin.bias_sigma.copy_(torch.tensor([1., 2.]))
    xo, xi = torch.tensor([2., -1.]), torch.tensor([1., 0., -2.])
    lin.set_noise(xo, xi)
    W, b = lin.effective()
    assert torch.equal(W, torch.tensor([[1 + .1 * 2, 2., 3 + .3 * -4], [4 + .4 * -1, 5., 6 + .6 * 2]]))
    assert torch.equal(b, torch.tensor([0.5 + 2., -0.5 - 2.]))
    x = torch.tensor([[1., 1., 1.], [0., 2., -1.]])
    y = lin(x)
    torch.testing.assert_close(y, x @ W.t() + b, rtol=0, atol=0)
    dy = torch.tensor([[1., -2.], [0.5, 3.]])
    (y * dy).sum().backward()
    dW = dy.t() @ x
    torch.testing.assert_close(lin.weight.grad, dW, rtol=0, atol=0)
    torch.testing.assert_close(lin.weight_sigma.grad, dW * torch.outer(xo, xi), rtol=0, atol=0)
    torch.testing.assert_close(lin.bias_sigma.grad, dy.sum(0) * xo, rtol=0, atol=0)


def test_zero_noise_is_the_plain_layer_and_init():
    torch.manual_seed(3)
    plain = torch.nn.Linear(12, 5)
    torch.manual_seed(3)
    lin = NoisyLinear(12, 5, sigma0=0.4)
    assert torch.equal(lin.weight, plain.weight) and torch.equal(lin.bias, plain.bias)
    x = torch.randn(7, 12)
    assert torch.equal(lin(x), plain(x))              # no noise set: zero noise
    lin.set_noise(torch.zeros(5), torch.zeros(12))
    assert torch.equal(lin(x), plain(x))
    s = 0.4 / np.sqrt(12)
    assert torch.equal(lin.weight_sigma, torch.full((5, 12), s)) and torch.equal(lin.bias_sigma, torch.full((5,), s))
    assert set(lin.state_dict()) == {"weight", "bias", "weight_sigma", "bias_sigma"}


@pytest.mark.parametrize("N", [1, 7])
def test_module_keys_shapes_and_mu_equal_to_the_plain_init(N):
    A = 3
    torch.manual_seed(1)
    plain = DuellingDQN((4, 84, 84), A, num_atoms=N)
    torch.manual_seed(1)
    net = DuellingDQN((4, 84, 84), A, num_atoms=N, noisy=True, noisy_sigma0=0.5)
    sd, ref = net.state_dict(), plain.state_dict()
    assert set(sd) == set(REFERENCE_KEYS) | set(SIGMA_KEYS)
    for k in REFERENCE_KEYS:
        assert torch.equal(sd[k], ref[k]), k
    for layer, p in zip(NOISY_LAYERS, (3136, 3136, 512, 512)):
        assert sd[f"{layer}.weight_sigma"].shape == sd[f"{layer}.weight"].shape
        assert sd[f"{layer}.bias_sigma"].shape == sd[f"{layer}.bias"].shape
        s0 = float(np.float32(0.5 / np.sqrt(p)))          # sigma0 / sqrt(fan-in), rounded to fp32
        assert float(sd[f"{layer}.weight_sigma"].unique()) == s0 and float(sd[f"{layer}.bias_sigma"].unique()) == s0
    x = torch.randint(0, 255, (2, 4, 84, 84), dtype=torch.uint8)
    with torch.no_grad():
        assert torch.equal(net(x)[2], plain(x)[2])    # zero noise
        net.set_noise(NZ.noise_vectors(SEED, 0, 0, A, N))
        assert not torch.equal(net(x)[2], plain(x)[2])
    mlp = build_network("mlp", [4], 2, noisy=True)
    assert isinstance(mlp, MLPDuellingDQN) and isinstance(mlp.value, NoisyLinear)
    with pytest.raises(ValueError, match="Runtime.noisy"):
        build_network("impala", [4, 84, 84], 4, noisy=True)


# ----------------------------------------------------------------- flat layout
# today's layout of the scalar head with 6 actions (asserted against the committed numbers)
OLD = {"w1": 0, "b1": 16384, "w2": 16448, "b2": 81984, "w3": 82048, "b3": 118912, "wv": 118976, "bv": 119488,
       "wa": 119552, "ba": 122624, "wfc": 122688, "bfc": 3333952}


@pytest.mark.parametrize("A,N", [(6, 1), (6, 51), (3, 7)])
def test_flat_layout_keeps_every_old_offset(A, N):
    old = FlatLayout(nature_segments(4, A, 64, N))
    same = FlatLayout(nature_segments(4, A, 64, N, noisy=False))
    assert old.offsets == same.offsets and old.numel == same.numel and old.segments == same.segments
    if (A, N) == (6, 1):
        assert old.offsets == OLD and old.numel == 3334976
    lay = FlatLayout(nature_segments(4, A, 64, N, noisy=True))
    assert [n for n, _ in lay.segments] == [n for n, _ in old.segments] + ["swv", "sbv", "swa", "sba", "swfc", "sbfc"]
    for k, o in old.offsets.items():
        assert lay.offsets[k] == o, k
    for m, s in NZ.SIGMA.items():
        assert lay.shapes[s] == lay.shapes[m] == old.shapes[m]
    assert lay.offsets["swv"] >= old.numel and lay.numel > old.numel + 1024 * 3136
    assert all(o % 64 == 0 for o in lay.offsets.values())


@pytest.mark.parametrize("c1,N", [(64, 1), (32, 7)])
def test_state_dict_flat_round_trip_with_sigma(c1, N):
    A = 5
    torch.manual_seed(2)
    net = DuellingDQN((4, 84, 84), A, conv1_channels=c1, num_atoms=N, noisy=True)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith("_sigma"):
                p.copy_(torch.rand_like(p))           # distinct values: a wrong permutation shows
    lay = FlatLayout(nature_segments(4, A, 64, N, noisy=True))
    flat = torch.zeros(lay.numel)
    v = lay.views(flat)
    reference_state_to_flat(net.state_dict(), v)
    back = flat_to_reference_state(v, c1)
    assert set(back) == set(net.state_dict())
    for k, t in net.state_dict().items():
        assert torch.equal(back[k], t), k
    # the fc sigma takes the fc weight's c,h,w -> h,w,c column permutation
    ws = net.state_dict()["advantage_stream_layer.0.weight_sigma"]
    assert float(v["swfc"][512 + 9, (3 * 7 + 2) * 64 + 17]) == float(ws[9, 17 * 49 + 3 * 7 + 2])
    assert float(v["sbfc"][512 + 9]) == float(net.state_dict()["advantage_stream_layer.0.bias_sigma"][9])
    # mismatches, both ways, before anything is copied
    plain = FlatLayout(nature_segments(4, A, 64, N))
    f2 = torch.full((plain.numel,), 7.0)
    with pytest.raises(ValueError, match="Runtime.noisy"):
        reference_state_to_flat(net.state_dict(), plain.views(f2))
    assert bool((f2 == 7.0).all())
    f3 = torch.full((lay.numel,), 7.0)
    with pytest.raises(ValueError, match="Runtime.noisy"):
        reference_state_to_flat(DuellingDQN((4, 84, 84), A, conv1_channels=c1, num_atoms=N).state_dict(), lay.views(f3))
    assert bool((f3 == 7.0).all())


# ----------------------------------------------------- fused backward vs autograd
def _setup(N=1, A=6, dist_head="categorical", B=8, **rt):
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": B},
                                "Runtime": {"grad_clip": 40.0, "network": "nature64", "presample": False,
                                            "num_atoms": N, "dist_head": dist_head, "noisy": True, **rt}})
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


@pytest.mark.parametrize("N,kind", [(1, "categorical"), (7, "categorical"), (7, "quantile")])
def test_fused_backward_matches_autograd(N, kind):
    """The bounds of tests/test_c51_cpu.py test_fused_backward_matches_autograd, over every mu
    and sigma segment; the module gets the draws the fused step composed with."""
    cfg, rp = _setup(N, dist_head=kind)
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.noisy and L.N == N and L.layout.numel > L.mu_layout.numel and not L._fuse_norm
    T = TorchLearner(cfg, "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    L._seg1()
    L._seg2()
    K = L._nz.K
    assert torch.equal(L.xi[0, :K], NZ.noise_vectors(L._nz.seed, 0, 0, L.A, N)["xi"].float())
    assert torch.equal(L.xi[1, :K], NZ.noise_vectors(L._nz.seed, 0, 1, L.A, N)["xi"].float())
    T.Q.set_noise(NZ.split_xi(L.xi[0], L.A, N))
    T.Q_target.set_noise(NZ.split_xi(L.xi[1], L.A, N))
    B, S = L.B, L.S
    batch = dict(S_t=L.frames[:B], S_tpn=L.frames[B:2 * B], A_t=S["act"], R=S["rew"], Gamma=S["gam"],
                 weights=S["weights"])
    lref, td = T.compute_loss_and_priorities(batch)
    T.optimizer.zero_grad()
    lref.backward()
    assert abs(float(lref) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref)))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    names = dict(T.Q.named_parameters())
    assert set(gf) == set(names) and set(SIGMA_KEYS) <= set(gf)
    for k, p in names.items():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")
    for k in SIGMA_KEYS:
        assert float(gf[k].abs().max()) > 0, k
    # the clip norm is the norm of the whole flat gradient, sigma included
    L._seg3()
    gn = float(L.g32.double().norm()) * L.is_scale()
    assert abs(float(L.gnorm) - gn) <= 1e-6 * gn
    o = L.layout.offsets
    assert float(L.g32[o["swv"]:].double().norm()) > 1e-3 * gn        # (and sigma carries a visible share of it)


# --------------------------------------------------------------- noise schedule
def test_noise_schedule_over_updates_and_target_sync():
    cfg, rp = _setup(1)
    cfg.Learner.q_target_sync_freq = 2
    L = FusedNatureLearner(cfg, "cpu", rp)
    K, seed = L._nz.K, L._nz.seed
    o = L.layout.offsets
    assert torch.equal(L.t32, L.p32)
    for u in range(2):
        assert L.update_index() == u
        p_before = L.p32.clone()
        L.step()
        on, tg = L.xi[0, :K].clone(), L.xi[1, :K].clone()
        # (the step composed at its head; a target sync recomposes for the next index afterwards)
        if L.num_q_updates % 2:
            assert torch.equal(on, NZ.noise_vectors(seed, u, 0, L.A, 1)["xi"].float())
            assert torch.equal(tg, NZ.noise_vectors(seed, u, 1, L.A, 1)["xi"].float())
            assert not torch.equal(on, tg)
        assert not torch.equal(p_before[o["swfc"]:], L.p32[o["swfc"]:])          # sigma is trained
    # two updates, one sync at the second: the target holds the online sigma
    assert L.num_q_updates == 2 and torch.equal(L.t32, L.p32)
    assert torch.equal(L.T["swfc"], L.P["swfc"]) and torch.equal(L.T["sbv"], L.P["sbv"])
    # the sync recomposed both nets with the draws of update 2
    assert torch.equal(L.xi[0, :K], NZ.noise_vectors(seed, 2, 0, L.A, 1)["xi"].float())
    m = L.last_metrics()
    assert np.isfinite(m["noisy_sigma_mean"]) and m["noisy_sigma_mean"] != 0.5 / np.sqrt(3136)


def test_effective_parameters_of_the_step_are_mu_plus_sigma_noise():
    cfg, rp = _setup(7)
    L = FusedNatureLearner(cfg, "cpu", rp)
    with torch.no_grad():
        L.P["swa"].mul_(3.0)
    L._noisy_compose()
    v = NZ.split_xi(L.xi[0].double(), L.A, 7)
    want = (L.P["wa"].double() + L.P["swa"].double() * torch.outer(v["a_out"], v["a_in"])).float()
    assert torch.equal(L.EP["wa"], want)
    want = (L.P["bfc"].double() + L.P["sbfc"].double() * v["fc_out"]).float()
    assert torch.equal(L.EP["bfc"], want)
    wfc = (L.P["wfc"].double() + L.P["swfc"].double() * NZ.outer(v, "wfc", (1024, 3136))).float()
    assert torch.equal(L.EPb["wfc"], wfc)        # (CPU, fp32 operands: one plane)
    assert L._head_params(L.P)["wa"] is L.EP["wa"] and L._head_params(L.T)["wa"] is L.ET["wa"]
    assert L._fc_weights()[0] is L.EPb["wfc"] and L._fc_weights()[3] is L.ETb["wfc"]


# ---------------------------------------------------------------------- config
def _cfg(**rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": rt})


@pytest.mark.parametrize("rt", [
    dict(noisy=True, network="impala"), dict(noisy=True, world_size=2), dict(noisy=True, force_dp=True),
    dict(noisy_sigma0=0.0), dict(noisy_sigma0=-1.0), dict(noisy=True, noisy_sigma0=0),
    dict(noisy_actor_resample=0), dict(noisy_actor_resample=-2), dict(noisy_actor_resample=1.5), dict(noisy=1),
])
def test_config_refusals(rt):
    with pytest.raises(ValueError, match="Runtime.noisy"):
        _cfg(**rt)


def test_config_defaults_head_kw_and_the_rainbow_config():
    import os
    c = _cfg()
    assert c.Runtime.noisy is False and c.Runtime.noisy_sigma0 == 0.5 and c.Runtime.noisy_actor_resample == 1
    assert "noisy" not in c.head_kw()
    n = _cfg(noisy=True, noisy_sigma0=0.25, noisy_actor_resample=3, num_atoms=51)
    assert n.head_kw()["noisy"] is True and n.head_kw()["noisy_sigma0"] == 0.25
    assert ApexConfig.from_dict(n.to_dict()).Runtime.noisy_actor_resample == 3
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                        "pong_1gpu_rainbow.json")
    r = ApexConfig.load(path).Runtime
    assert r.noisy and r.num_atoms == 51 and r.optimizer == "adam" and r.is_beta_end == 1.0


def test_learners_without_noisy_layers_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    cfg, rp = _setup(1)
    with pytest.raises(ValueError, match="Runtime.noisy"):
        GraphLearner(cfg, "cpu", rp)

    class Comm:                      # a second rank: the data-parallel step
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="Runtime.noisy"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_mismatches_round_trip_and_resume(tmp_path):
    cfg, rp = _setup(7)
    L = FusedNatureLearner(cfg, "cpu", rp)
    L.step()
    L.step()
    path = str(tmp_path / "noisy.pt")
    L.save(path)
    cfg2, rp2 = _setup(7)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    assert not torch.equal(L.p32, L2.p32)
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits), (rp.leaf, rp.nodes, rp.min_bits)):
        dst.copy_(src)              # (the replay is not part of a checkpoint: the same priorities)
    assert L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.pbf, L2.pbf)):
        assert torch.equal(a, b)
    assert L2.num_q_updates == 2 and L2.update_index() == 2
    # the restored learner composed the draws of update 2, and resumes to identical parameters
    assert torch.equal(L2.xi[0, :L._nz.K], NZ.noise_vectors(L._nz.seed, 2, 0, L.A, 7)["xi"].float())
    assert torch.equal(L2.xi[1, :L._nz.K], NZ.noise_vectors(L._nz.seed, 2, 1, L.A, 7)["xi"].float())
    for X in (L, L2):
        X.step()
        X.step()
    assert torch.equal(L.p32, L2.p32) and torch.equal(L.rms_v, L2.rms_v) and torch.equal(L.t32, L2.t32)
    # a noisy checkpoint into a non-noisy learner
    cfg3, rp3 = _setup(7, noisy=False)
    L3 = FusedNatureLearner(cfg3, "cpu", rp3)
    p3 = L3.p32.clone()
    with pytest.raises(ValueError, match="Runtime.noisy"):
        L3.load(path)
    assert torch.equal(p3, L3.p32)
    # a non-noisy checkpoint (and a reference state dict, which has no sigma) into a noisy learner
    plain = str(tmp_path / "plain.pt")
    L3.save(plain)
    p0 = L.p32.clone()
    with pytest.raises(ValueError, match="Runtime.noisy"):
        L.load(plain)
    with pytest.raises(ValueError, match="Runtime.noisy"):
        L.load_reference_state_dict(DuellingDQN((4, 84, 84), 6, num_atoms=7).state_dict())
    assert torch.equal(p0, L.p32)
    # the optimizer state is tagged per segment, sigma segments included
    ck = torch.load(path, weights_only=True)
    assert {"swfc", "sbfc", "swv", "swa"} <= {n for n, _, _ in ck["optimizer_state"]["layout"]}
    assert set(SIGMA_KEYS) <= set(ck["Q_state"]) and set(SIGMA_KEYS) <= set(ck["Q_target_state"])
    # the torch learner refuses the same mismatches
    tl = TorchLearner(cfg3, "cpu")
    with pytest.raises(ValueError, match="Runtime.noisy"):
        tl.load(path)


# --------------------------------------------------------------- torch learner
def test_mlp_torch_learner_with_noisy_layers():
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 1000},
                                "Runtime": {"noisy": True, "lr": 1e-3}})
    T = TorchLearner(cfg, "cpu")
    assert isinstance(T.Q.value, NoisyLinear) and isinstance(T.Q.value_stream_layer[0], NoisyLinear)
    s0 = T.Q.value_stream_layer[0].weight_sigma.detach().clone()
    g = torch.Generator().manual_seed(3)
    B = 32
    batch = dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                 A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g) * 3,
                 Gamma=torch.full((B,), 0.97), weights=torch.rand(B, generator=g) + 0.5)
    draws = []
    for u in range(4):
        out = T.step(batch)
        assert np.isfinite(out["loss"]) and np.isfinite(out["td_abs"]).all()
        draws.append((T.Q.value.xi_in.clone(), T.Q_target.value.xi_in.clone()))
        want = NZ.noise_vectors(SEED, u, 0, 2, 1, hidden=128, fc_in=128)
        assert torch.equal(draws[-1][0], want["v_in"].float())
        assert torch.equal(T.Q.value_stream_layer[0].xi_out, want["fc_out"][:128].float())
        assert torch.equal(draws[-1][1], NZ.noise_vectors(SEED, u, 1, 2, 1, hidden=128, fc_in=128)["v_in"].float())
    assert not torch.equal(draws[0][0], draws[1][0]) and not torch.equal(draws[0][0], draws[0][1])
    assert not torch.equal(s0, T.Q.value_stream_layer[0].weight_sigma)
    assert T.num_q_updates == 4


def test_inline_training_runs_with_noisy_actors():
    from apex_dqn_amd.runtime.loops import train_inline
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Actor": {"num_actors": 4, "Q_network_sync_freq": 5},
                                "Learner": {"min_replay_mem_size": 32, "replay_sample_size": 16},
                                "Runtime": {"noisy": True, "noisy_actor_resample": 3}})
    out = train_inline(cfg, 6, max_actor_steps=400)
    assert out["learner"].num_q_updates == 6 and np.isfinite(out["losses"]).all()
