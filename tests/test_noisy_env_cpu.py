"""Per-environment actor noise (Runtime.noisy_actor_noise = "per_env") on the CPU: the host mirror, the
torch-backend oracles in fp64 against the noisy module evaluated one env at a time, a GpuActorGroup on the torch
backend, the key's validation and the refusals."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import noisy as NZ
from apex_dqn_amd.models.dueling import DuellingDQN
from apex_dqn_amd.ops.fused_ops import TorchBackend

SEED = NZ.noise_seed(0)


def test_mirror_row_zero_is_the_shared_draw_and_rows_differ():
    A, N, u, s = 3, 7, 5, 4
    rows = [NZ.env_noise_vectors(SEED, u, s, e, A, N)["xi"] for e in range(4)]
    assert torch.equal(rows[0], NZ.noise_vectors(SEED, u, s, A, N)["xi"])
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(rows[i], rows[j])
            assert float((rows[i] - rows[j]).abs().mean()) > 0.5         # other values throughout


@pytest.mark.parametrize("A,N,kind", [(4, 1, "scalar"), (3, 7, "quantile"), (4, 11, "categorical")])
def test_torch_ops_fp64_vs_module_one_env_at_a_time(A, N, kind):
    """draw -> noisy_env_fc -> noisy_env_logits -> finish in fp64 == q of models/dueling.py's noisy module with
    set_noise(env_noise_vectors(e)) on row e, within the 1e-12 this suite applies to fp64 oracles."""
    E, u, s = 3, 2, 3
    torch.manual_seed(1)
    net = DuellingDQN((4, 84, 84), A, noisy=True, num_atoms=N, v_min=-2.0, v_max=3.0,
                      dist_head="quantile" if kind == "quantile" else "categorical").double()
    with torch.no_grad():
        for m in (net.value_stream_layer[0], net.advantage_stream_layer[0], net.value, net.advantage):
            m.weight_sigma.copy_(torch.rand_like(m.weight_sigma) * 0.05)
            m.bias_sigma.copy_(torch.rand_like(m.bias_sigma) * 0.05)
    X = torch.rand(E, 3136, dtype=torch.float64)                          # the engine's h, w, c column order
    x_mod = X.reshape(E, 7, 7, 64).permute(0, 3, 1, 2).reshape(E, -1)
    eng = lambda w: w.reshape(512, 64, 7, 7).permute(0, 2, 3, 1).reshape(512, 3136)      # noqa: E731
    lv, la = net.value_stream_layer[0], net.advantage_stream_layer[0]
    w, sw = (torch.cat([eng(getattr(lv, k)), eng(getattr(la, k))]).detach() for k in ("weight", "weight_sigma"))
    b, sb = (torch.cat([getattr(lv, k), getattr(la, k)]).detach() for k in ("bias", "bias_sigma"))
    P = {"wv": net.value.weight.detach(), "bv": net.value.bias.detach(), "wa": net.advantage.weight.detach(),
         "ba": net.advantage.bias.detach()}
    S = {"wv": net.value.weight_sigma.detach(), "bv": net.value.bias_sigma.detach(),
         "wa": net.advantage.weight_sigma.detach(), "ba": net.advantage.bias_sigma.detach()}
    ops = TorchBackend()
    ctr = torch.tensor([u], dtype=torch.int64)
    plan = NZ.NoisyPlan(A=A, N=N, offsets={}, seed=SEED, ctr=ctr, stream0=s)
    xi = torch.zeros(E, plan.K, dtype=torch.float64)
    h = torch.zeros(E, 1024, dtype=torch.float64)
    L = ops.noisy_env_logits_ws(E, A, N, "cpu", dtype=torch.float64)
    q, act = torch.zeros(E, A, dtype=torch.float64), torch.zeros(E, dtype=torch.int32)
    ops.noisy_env_draw(plan, xi)
    ops.noisy_env_fc(X, w, sw, b, sb, xi, h)
    ops.noisy_env_logits(h, P, S, xi, N, L)
    head = {"scalar": ("scalar",), "quantile": ("quantile", N), "categorical": ("categorical", N, -2.0, 3.0)}[kind]
    ops.noisy_env_finish(h, L, P, torch.zeros(E), ctr, 0, head, q, act)
    for e in range(E):
        net.set_noise(NZ.env_noise_vectors(SEED, u, s, e, A, N))
        with torch.no_grad():
            hv, ha = lv(x_mod[e:e + 1]).relu(), la(x_mod[e:e + 1]).relu()
            q_ref = net._head(hv, ha)[2][0]
        assert float((torch.cat([hv, ha], 1)[0] - h[e]).abs().max()) <= 1e-12
        assert float((q[e] - q_ref).abs().max()) <= 1e-12, (e, q[e], q_ref)
        assert int(act[e]) == int(q_ref.argmax())
    assert float((q[0] - q[1]).abs().max()) > 1e-6


def _cfg(**rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Actor": {"num_actors": 3, "epsilon": 0.0}, "Learner": {"replay_sample_size": 8},
                                 "Runtime": {"noisy": True, "presample": False, **rt}})


@pytest.mark.parametrize("mode", ["per_env", "shared"])
def test_actor_group_identical_frames(mode):
    """Every env sees the same frame stack: q rows differ under "per_env" and are identical under "shared"."""
    from apex_dqn_amd.actors.gpu_actor import GpuActorGroup
    from apex_dqn_amd.envs.vector_envs import make_vec_env
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    E = 3
    cfg = _cfg(noisy_actor_noise=mode, num_atoms=7, dist_head="quantile")
    torch.manual_seed(0)
    rp = GpuReplayShard(400, 400, 600, 4, device="cpu")
    L = FusedNatureLearner(cfg, "cpu", rp)
    grp = GpuActorGroup(cfg, L, rp, make_vec_env(cfg.env_backend, cfg.env_conf.name, E, 4, seed=0), E, group=1)
    assert grp.env_noise == (mode == "per_env") and grp.xi.shape[0] == (E if grp.env_noise else 1)
    seqs = rp.append_frames(np.random.default_rng(0).integers(0, 255, (4, 84, 84), dtype=np.uint8))
    q, _ = grp.policy(np.repeat(seqs[None, :], E, axis=0))
    assert np.isfinite(q).all() and int(grp.ctr) == 1
    if mode == "shared":
        assert np.array_equal(q[0], q[1]) and np.array_equal(q[0], q[2])
    else:
        assert min(np.abs(q[i] - q[j]).max() for i, j in ((0, 1), (0, 2), (1, 2))) > 1e-6
        assert torch.equal(grp.xi[0, :grp._nz.K], NZ.noise_vectors(grp._nz.seed, 0, 3, 4, 7)["xi"].float())


def test_key_validation_and_refusals():
    assert _cfg().Runtime.noisy_actor_noise == "shared"
    assert _cfg(noisy_actor_noise="per_env").Runtime.noisy_actor_noise == "per_env"
    with pytest.raises(ValueError, match="noisy_actor_noise"):
        _cfg(noisy_actor_noise="per_actor")
    with pytest.raises(ValueError, match="noisy_actor_noise"):
        _cfg(noisy_actor_noise="per_env", layer_norm=True)
    with pytest.raises(ValueError, match="noisy_actor_noise"):         # the CPU actor groups and the inline loop
        NZ.actor_noise_hook(_cfg(noisy_actor_noise="per_env"), None, 0)
    assert NZ.actor_noise_hook(_cfg(noisy=False, noisy_actor_noise="per_env"), None, 0) is None      # no effect
