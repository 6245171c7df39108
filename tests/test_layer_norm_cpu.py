"""Runtime.layer_norm on the CPU: the config, the modules' keys, the flat layout, the fp64 oracle against autograd
through nn.LayerNorm, a torch-backend learner step against autograd on the module, the reset rows, checkpoints."""
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.graph_learner import GraphLearner
from apex_dqn_amd.models.dueling import LN_KEYS, REFERENCE_KEYS, build_network
from apex_dqn_amd.models.flat_params import FlatLayout, nature_segments
from test_fused_learner_cpu import _setup


def _cfg(shape=(4, 84, 84), **rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": list(shape), "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": {"layer_norm": True, **rt}})


@pytest.mark.parametrize("key,make", [("layer_norm_eps", lambda e=e: _cfg(layer_norm_eps=e))
                                      for e in (0.0, -1e-5, float("inf"), float("nan"), True, "1e-5")]
                         + [("layer_norm", lambda rt=rt: _cfg(**rt)) for rt in (dict(network="impala"), dict(world_size=2), dict(force_dp=True))]
                         + [("layer_norm", lambda: GraphLearner(_cfg(), "cpu", None))])
def test_refusals_name_the_key(key, make):
    with pytest.raises(ValueError, match="Runtime." + key):
        make()


@pytest.mark.parametrize("kind,shape,width", [("nature64", (4, 84, 84), 512), ("mlp", (4,), 128)])
def test_module_keys_and_initial_values(kind, shape, width):
    cfg = _cfg(shape)
    sd, plain = build_network(kind, shape, 4, **cfg.head_kw()).state_dict(), build_network(kind, shape, 4).state_dict()
    assert set(sd) == set(plain) | set(LN_KEYS) and (kind == "mlp" or set(REFERENCE_KEYS) <= set(sd))
    for k in LN_KEYS:
        assert sd[k].shape == (width,) and bool((sd[k] == (1.0 if k.endswith("weight") else 0.0)).all())
    assert "layer_norm" not in ApexConfig.from_dict({"env_conf": cfg.to_dict()["env_conf"]}).head_kw()


@pytest.mark.parametrize("kw", [dict(), dict(noisy=True), dict(implicit=True), dict(num_atoms=5)])
def test_layout_keeps_every_offset(kw):
    off, on = FlatLayout(nature_segments(4, 6, **kw)), FlatLayout(nature_segments(4, 6, layer_norm=True, **kw))
    assert [s for s, _ in on.segments] == [s for s, _ in off.segments] + ["lng", "lnb"]
    assert all(on.offsets[k] == o for k, o in off.offsets.items()) and on.offsets["lng"] >= off.numel


def test_oracle_matches_autograd_through_nn_layernorm():
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    g = torch.Generator().manual_seed(0)
    M, F, eps = 5, 512, 1e-5
    a = (torch.randn(M, 2 * F, generator=g, dtype=torch.float64) * 3 + 1).requires_grad_(True)
    ln = [torch.nn.LayerNorm(F, eps=eps).double() for _ in range(2)]
    for m in ln:
        m.weight.data = torch.rand(F, generator=g, dtype=torch.float64) + 0.5
        m.bias.data = torch.randn(F, generator=g, dtype=torch.float64)
    gamma, beta = torch.cat([m.weight for m in ln]).detach(), torch.cat([m.bias for m in ln]).detach()
    h_ref = torch.relu(torch.cat([ln[0](a[:, :F]), ln[1](a[:, F:])], 1))
    h, xh, r = TorchBackend.fc_ln_fwd(a.detach(), gamma, beta, eps)
    torch.testing.assert_close(h, h_ref, rtol=1e-12, atol=1e-12)
    up = torch.randn(M, 2 * F, generator=g, dtype=torch.float64)
    (h_ref * up).sum().backward()
    da, gg, gb = TorchBackend.fc_ln_bwd(up * (h > 0), xh, r, gamma)
    for got, ref in ((da, a.grad), (gg, torch.cat([m.weight.grad for m in ln])), (gb, torch.cat([m.bias.grad for m in ln]))):
        torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-12)


def _on(cfg, rp, **rt):
    return ApexConfig.from_dict({**cfg.to_dict(), "Runtime": {**cfg.to_dict()["Runtime"], "layer_norm": True, **rt}}), rp


def _learner(**rt):
    cfg, rp = _on(*_setup(), **rt)
    return cfg, FusedNatureLearner(cfg, "cpu", rp)


def test_torch_backend_step_matches_autograd_on_the_module(monkeypatch):
    """tests/test_fused_learner_cpu.py ``_check`` (its tolerances, every module parameter) with the flag on."""
    import test_fused_learner_cpu as ref
    monkeypatch.setattr(ref, "_setup", lambda *a, **k: _on(*_setup(*a, **k)))
    L = ref._check("huber")
    assert L.layer_norm and not L._fuse_norm and not L._defer_fc_epilogue and "ln_rstd_mean" in L.last_metrics()
    assert float(L.G["lng"].abs().max()) > 0 and float(L.G["lnb"].abs().max()) > 0


def test_reset_rows_and_reset_now():
    cfg, L = _learner(reset_interval=5, reset_shrink_head=0.25)
    rows = {(r.start, r.end): r for r in L._reset_table}
    for name, const in (("lng", 1.0), ("lnb", 0.0)):
        r = rows[(L.layout.offsets[name], L.layout.offsets[name] + 1024)]
        assert (r.const_flag, r.const_value, r.alpha, r.period, r.live) == (1, const, 0.25, 1024, 1024)
    L.p32[L.layout.offsets["lng"]:].fill_(3.0)      # lng and lnb, the last two segments; the target the same
    L.sync_target()
    L.reset_now(1)
    for V in (L.P, L.T):       # alpha old + (1 - alpha) const
        assert bool((V["lng"] == 0.25 * 3.0 + 0.75).all()) and bool((V["lnb"] == 0.75).all())


def test_checkpoint_round_trip_and_cross_refusals(tmp_path):
    cfg, L = _learner()
    L.P["lng"].uniform_(0.5, 1.5)
    L.T["lnb"].uniform_(-1, 1)
    on, off = str(tmp_path / "on.pt"), str(tmp_path / "off.pt")
    L.save(on)
    L2 = FusedNatureLearner(cfg, "cpu", L.replay)
    assert L2.load(on) and torch.equal(L2.p32, L.p32) and torch.equal(L2.t32, L.t32)
    plain_cfg, rp = _setup()
    plain = FusedNatureLearner(plain_cfg, "cpu", rp)
    plain.save(off)
    for bad in (lambda: plain.load(on), lambda: L2.load(off), lambda: L2.load_reference_state_dict(plain.reference_state_dict())):
        with pytest.raises(ValueError, match="Runtime.layer_norm"):
            bad()
