"""Random-shift (DrQ) frame augmentation on the CPU: the host mirror (learner/augment.py) against
an independent definition, the config key, the fused learner on the torch backend against
autograd on explicitly shifted images, the Munchausen row plan, off-is-off, continuity over
updates and checkpoints, and the torch learner."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import augment as AU
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.flat_params import flat_to_reference_state
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

M64 = (1 << 64) - 1


# ------------------------------------------------------------------- 1. shift_frames
def _pad_crop(x, oy, ox, P):
    """The independent definition: replicate-pad by P, crop 84 x 84 at (oy, ox)."""
    return F.pad(x.float(), (P, P, P, P), mode="replicate")[..., oy:oy + 84, ox:ox + 84].to(torch.uint8)


@pytest.mark.parametrize("P,pairs", [
    (1, [(oy, ox) for oy in range(3) for ox in range(3)]),
    (4, [(0, 0), (0, 8), (8, 0), (8, 8), (4, 4)]),
    (8, [(0, 0), (0, 16), (16, 0), (16, 16), (8, 8)]),
])
def test_shift_frames_is_replicate_pad_and_crop(P, pairs):
    g = torch.Generator().manual_seed(P)
    x = torch.randint(0, 256, (len(pairs), 3, 84, 84), dtype=torch.uint8, generator=g)
    off = torch.tensor(pairs, dtype=torch.int32)
    y = AU.shift_frames(x, off, P)
    assert y.dtype == torch.uint8 and y.shape == x.shape and y.is_contiguous()
    for r, (oy, ox) in enumerate(pairs):
        assert torch.equal(y[r], _pad_crop(x[r], oy, ox, P)), (P, oy, ox)
        if (oy, ox) == (P, P):
            assert torch.equal(y[r], x[r])          # the centre offset is the identity
        else:
            assert not torch.equal(y[r], x[r])


# ------------------------------------------------------------------ 2. shift_offsets
def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _k24(seed, ctr, i):
    """apex_uniform(seed, ctr, i) 2^24 in Python integers (csrc/apex_common.h, by hand)."""
    return _mix(seed ^ _mix((ctr * 0x100000001B3 + i) & M64)) >> 40


def test_shift_offsets_by_hand_range_determinism_and_keys():
    sa = AU.aug_seed(0)
    for (u, r, P) in [(0, 0, 4), (3, 5, 1), (1000, 511, 8)]:
        want = [(_k24(sa, 64 * u, 2 * r + ax) * (2 * P + 1)) >> 24 for ax in (0, 1)]
        got = AU.shift_offsets(sa, u, r + 1, P)
        assert got.dtype == torch.int32 and tuple(got.shape) == (r + 1, 2)
        assert got[r].tolist() == want, (u, r, P)
    for P in (1, 4, 8):
        o = AU.shift_offsets(sa, 7, 1024, P)
        assert int(o.min()) == 0 and int(o.max()) == 2 * P
        assert torch.equal(o, AU.shift_offsets(sa, 7, 1024, P))
        assert not torch.equal(o, AU.shift_offsets(sa, 8, 1024, P))
        assert not torch.equal(o, AU.shift_offsets(AU.aug_seed(1), 7, 1024, P))
        # a longer batch extends a shorter one: row r does not depend on the batch size
        assert torch.equal(o[:100], AU.shift_offsets(sa, 7, 100, P))
    for bad in (0, 9, -1, True, 2.0):
        with pytest.raises(ValueError):
            AU.shift_offsets(sa, 0, 4, bad)


def test_shift_offsets_are_uniform():
    """2 x 4096 draws at P = 4: every one of the 9 bins within 5 sigma of n / 9 (binomial)."""
    o = AU.shift_offsets(AU.aug_seed(0), 11, 4096, 4).reshape(-1)
    n = o.numel()
    assert n == 8192
    cnt = np.bincount(o.numpy(), minlength=9)
    p = 1.0 / 9.0
    sigma = np.sqrt(n * p * (1 - p))
    assert cnt.sum() == n and len(cnt) == 9
    assert np.abs(cnt - n * p).max() <= 5 * sigma, cnt


def test_aug_seed_is_its_own_stream():
    from apex_dqn_amd.learner.iqn import iqn_seed
    from apex_dqn_amd.learner.noisy import noise_seed
    for s in (0, 1, 1234, 2 ** 40 + 3):
        a = AU.aug_seed(s)
        assert 0 <= a < 2 ** 63 and a == AU.aug_seed(s)
        assert len({a, noise_seed(s), iqn_seed(s), s}) == 4
        assert a == _mix((s ^ 0x4472517368696674) & M64) & (2 ** 63 - 1)
    assert AU.aug_seed(0) != AU.aug_seed(1)


# ----------------------------------------------------------------- 3. aug_slot_table
@pytest.mark.parametrize("B,C", [(8, 4), (3, 2), (1, 1)])
def test_aug_slot_table(B, C):
    d = AU.aug_slot_table(B, C, False)
    m = AU.aug_slot_table(B, C, True)
    want = torch.arange(2 * B * C, dtype=torch.int32).reshape(2 * B, C)
    for t in (d, m):
        assert t.dtype == torch.int32 and tuple(t.shape) == (3 * B, C) and t.is_contiguous()
        assert torch.equal(t[:2 * B], want)
        assert int(t.max()) == 2 * B * C - 1 and int(t.min()) == 0
    assert torch.equal(d[2 * B:], want[B:])         # default plan: the target net at S_t+n
    assert torch.equal(m[2 * B:], want[:B])         # Munchausen plan: the target net at S_t


# ------------------------------------------------------------------------ 4. config
def _cfg(ss=(4, 84, 84), **rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": list(ss), "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": rt})


def test_config_default_and_range():
    assert _cfg().Runtime.augment_shift == 0
    for P in range(0, 9):
        c = _cfg(augment_shift=P)
        assert c.Runtime.augment_shift == P
        assert ApexConfig.from_dict(c.to_dict()).Runtime.augment_shift == P
    assert _cfg(augment_shift=4, network="nature32").network == "nature32"
    # it composes with every head kind and the other single-rank features
    _cfg(augment_shift=4, num_atoms=51, noisy=True, optimizer="adam", target_ema_rate=0.01, value_rescale=True)
    _cfg(augment_shift=4, num_atoms=32, dist_head="quantile", dtype="bf16", presample=False)
    _cfg(augment_shift=4, num_atoms=32, dist_head="implicit")
    _cfg(augment_shift=4, munchausen=True, lr_warmup_steps=10)
    _cfg(ss=(4,), augment_shift=0)


@pytest.mark.parametrize("kw", [
    dict(augment_shift=True), dict(augment_shift=False), dict(augment_shift=9), dict(augment_shift=-1),
    dict(augment_shift=2.0), dict(augment_shift="4"),
    dict(augment_shift=4, network="impala"), dict(augment_shift=4, network="mlp"),
    dict(augment_shift=1, world_size=2), dict(augment_shift=1, force_dp=True),
    dict(ss=(4,), augment_shift=4), dict(ss=(4, 64, 64), augment_shift=4, network="impala"),
])
def test_config_refusals(kw):
    with pytest.raises(ValueError, match="Runtime.augment_shift"):
        _cfg(**kw)


def test_config_refuses_other_frame_sizes():
    # (NatureCNN itself needs 84 x 84; the key's own check fires first and names the key)
    with pytest.raises(ValueError, match="Runtime.augment_shift"):
        _cfg(ss=(4, 96, 96), augment_shift=2, network="nature64")


def test_pong_drq_config():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = ApexConfig.load(os.path.join(root, "configs", "pong_1gpu_drq.json"))
    base = ApexConfig.load(os.path.join(root, "configs", "pong_1gpu.json"))
    assert c.Runtime.augment_shift == 4 and c.Runtime.optimizer == "adam" and c.Runtime.num_atoms == 1
    assert c.Actor.num_steps == base.Actor.num_steps and c.network in ("nature64", "nature32")


# ------------------------------------------- 5. the fused learner on the torch backend
def _setup(N=1, A=6, dist_head="categorical", B=8, P=4, seed=0, **rt):
    torch.manual_seed(0)
    rtd = {"grad_clip": 40.0, "network": "nature64", "presample": False, "num_atoms": N, "dist_head": dist_head,
           "seed": seed, **rt}
    if P is not None:
        rtd["augment_shift"] = P
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": B}, "Runtime": rtd})
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


def _plain(cfg):
    """The same config with the key off: a torch learner that shifts nothing itself."""
    d = cfg.to_dict()
    d["Runtime"]["augment_shift"] = 0
    return ApexConfig.from_dict(d)


def _shifted_batch(L, u, shift=True):
    """S_t / S_t+n of the learner's sampled rows, gathered from the ring and shifted explicitly by
    the mirror's offsets for update ``u`` (or left as they are)."""
    B, S, P = L.B, L.S, L.aug_pad
    raw = L.replay.gather_frames(L.slots[:2 * B])
    if shift:
        off = AU.shift_offsets(AU.aug_seed(L.rt.seed), u, 2 * B, P)
        raw = AU.shift_frames(raw, off, P)
    return dict(S_t=raw[:B], S_tpn=raw[B:], A_t=S["act"], R=S["rew"], Gamma=S["gam"], weights=S["weights"])


def _autograd(cfg, L, batch):
    T = TorchLearner(_plain(cfg), "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    lref, td = T.compute_loss_and_priorities(batch)
    T.optimizer.zero_grad()
    lref.backward()
    return lref, td, dict(T.Q.named_parameters())


def _check_grads(cfg, L, seed=0):
    """tests/test_noisy_cpu.py test_fused_backward_matches_autograd's bounds: loss 1e-5 relative, td_abs and
    gradients at rtol 1e-4 (1e-5 for td) with its atol."""
    B, P = L.B, L.aug_pad
    off = AU.shift_offsets(AU.aug_seed(seed), 0, 2 * B, P)
    assert torch.equal(L.aug_off, off)
    assert float((off - P).abs().max()) > 0             # (some row is really shifted)
    lref, td, names = _autograd(cfg, L, _shifted_batch(L, 0))
    lref = lref.detach()
    assert abs(float(lref) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref)))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    assert set(gf) == set(names)
    for k, p in names.items():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")
    # ... and it is not the gradient on the unshifted images
    l0, td0, names0 = _autograd(cfg, L, _shifted_batch(L, 0, shift=False))
    k = "conv1.weight" if "conv1.weight" in names0 else next(n for n in names0 if n.endswith("weight"))
    rel = float((gf[k] - names0[k].grad).norm() / names0[k].grad.norm())
    assert rel > 1e-2, rel
    assert float((td0 - L.td_abs).abs().max()) > 1e-4
    return off


@pytest.mark.parametrize("N,kind", [(1, "categorical"), (7, "quantile")])
def test_fused_backward_matches_autograd_on_shifted_images(N, kind):
    cfg, rp = _setup(N, dist_head=kind)
    L = FusedNatureLearner(cfg, "cpu", rp)
    B, C = L.B, L.C
    assert L.aug_pad == 4 and tuple(L.aug_frames.shape) == (2 * B * C, 84, 84) and L.aug_frames.dtype == torch.uint8
    assert torch.equal(L.aug_slots, AU.aug_slot_table(B, C, False)) and tuple(L.aug_off.shape) == (2 * B, 2)
    ring, slots = L._frame_src()
    assert ring is L.aug_frames and slots is L.aug_slots
    L._seg1()
    L._seg2()
    off = _check_grads(cfg, L)
    # the forward's rows: S_t, S_t+n, and the target rows see the S_t+n copy (not a third shift)
    raw = rp.gather_frames(L.slots[:2 * B])
    sh = AU.shift_frames(raw, off, 4)
    assert torch.equal(L.frames[:2 * B], sh)
    assert torch.equal(L.frames[2 * B:], sh[B:])
    assert torch.equal(L.slots[2 * B:], L.slots[B:2 * B])      # (the sampler still writes its slots)
    # the buffer is in the ring's layout
    from apex_dqn_amd.replay.gpu_replay import to_s2d
    assert torch.equal(L.aug_frames, to_s2d(sh.reshape(2 * B * C, 84, 84)))
    L._seg3()
    m = L.last_metrics()
    assert m["augment_offset_mean"] == float(off.double().mean()) and 0 <= m["augment_offset_mean"] <= 8


# --------------------------------------------------------- 6. the Munchausen row plan
def test_munchausen_row_plan_reads_the_s_t_copy():
    cfg, rp = _setup(1, munchausen=True)
    L = FusedNatureLearner(cfg, "cpu", rp)
    B = L.B
    assert L.munchausen and torch.equal(L.aug_slots, AU.aug_slot_table(B, L.C, True))
    L._seg1()
    L._seg2()
    off = _check_grads(cfg, L)
    sh = AU.shift_frames(rp.gather_frames(L.slots[:2 * B]), off, 4)
    assert torch.equal(L.frames[:2 * B], sh)
    assert torch.equal(L.frames[2 * B:], sh[:B])               # the target net at S_t: the S_t copy
    assert torch.equal(L.slots[2 * B:], L.slots[:B])


# ------------------------------------------------------------------- 7. off is off
def test_off_is_off():
    res = []
    for P in (0, None):
        cfg, rp = _setup(1, P=P)
        L = FusedNatureLearner(cfg, "cpu", rp)
        assert L.aug_pad == 0 and L.aug_frames is None and L.aug_slots is None and L.aug_off is None
        ring, slots = L._frame_src()
        assert ring is rp.frames and slots is L.slots
        for _ in range(3):
            L.step()
        assert "augment_offset_mean" not in L.last_metrics()
        res.append((L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.g32.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # ... and on is not off
    cfg, rp = _setup(1, P=4)
    L = FusedNatureLearner(cfg, "cpu", rp)
    for _ in range(3):
        L.step()
    assert not torch.equal(L.p32, res[0][0])


def test_learners_without_augmentation_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    from apex_dqn_amd.learner.impala_learner import FusedImpalaLearner
    cfg, rp = _setup(1)
    with pytest.raises(ValueError, match="Runtime.augment_shift"):
        GraphLearner(cfg, "cpu", rp)
    with pytest.raises(ValueError, match="Runtime.augment_shift"):
        FusedImpalaLearner(cfg, "cpu", rp)

    class Comm:                      # a second rank: the data-parallel step
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="Runtime.augment_shift"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


# ------------------------------------------------ 8. continuity and checkpoints
@pytest.mark.parametrize("presample", [False, True])
def test_offsets_follow_the_update_index(presample):
    cfg, rp = _setup(1, presample=presample, seed=3)
    L = FusedNatureLearner(cfg, "cpu", rp)
    sa = AU.aug_seed(3)
    seen = []
    for u in range(4):
        assert L.update_index() == u
        L.step()
        assert torch.equal(L.aug_off, AU.shift_offsets(sa, u, 2 * L.B, 4)), (presample, u)
        seen.append(L.aug_off.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[2], seen[3])


def test_resume_and_checkpoints_across_the_setting(tmp_path):
    cfg, rp = _setup(1)
    L = FusedNatureLearner(cfg, "cpu", rp)
    for _ in range(3):
        L.step()
    path = str(tmp_path / "aug.pt")
    L.save(path)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(3):
        L.step()
    cfg2, rp2 = _setup(1)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)              # (the replay is not part of a checkpoint: the same priorities and counter)
    assert L2.load(path)
    assert L2.num_q_updates == 3 and L2.update_index() == 3
    for _ in range(3):
        L2.step()
    assert torch.equal(L2.aug_off, AU.shift_offsets(AU.aug_seed(0), 5, 2 * L.B, 4))
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (rp.leaf, rp2.leaf),
                 (L.aug_off, L2.aug_off), (L.aug_frames, L2.aug_frames)):
        assert torch.equal(a, b)
    # the checkpoint gained no keys ...
    ck = torch.load(path, weights_only=True)
    cfg0, rp0 = _setup(1, P=0)
    L0 = FusedNatureLearner(cfg0, "cpu", rp0)
    L0.step()
    plain = str(tmp_path / "plain.pt")
    L0.save(plain)
    ck0 = torch.load(plain, weights_only=True)
    assert set(ck) == set(ck0) and set(ck["Q_state"]) == set(ck0["Q_state"])
    # ... and loads across the setting, both ways
    assert L0.load(path)
    sd = flat_to_reference_state(L0.P, L0.c1)
    for k, v in ck["Q_state"].items():
        assert torch.equal(sd[k], v), k
    assert L0.num_q_updates == 3 and L0.aug_frames is None
    L0.step()
    cfg3, rp3 = _setup(1)
    L3 = FusedNatureLearner(cfg3, "cpu", rp3)
    assert L3.load(plain) and L3.num_q_updates == 1 and L3.update_index() == 1
    L3.step()
    assert torch.equal(L3.aug_off, AU.shift_offsets(AU.aug_seed(0), 1, 2 * L3.B, 4))


# --------------------------------------------------------------- 9. the torch learner
@pytest.mark.parametrize("N,kind,mdqn", [(1, "categorical", False), (7, "quantile", False), (1, "categorical", True)])
def test_torch_learner_shifts_an_84x84_batch(N, kind, mdqn):
    torch.manual_seed(0)
    rt = {"network": "nature64", "num_atoms": N, "dist_head": kind, "munchausen": mdqn, "seed": 2}
    env = {"state_shape": [4, 84, 84], "action_dim": 5, "name": "Synthetic"}
    cfg = ApexConfig.from_dict({"env_conf": env, "Runtime": {**rt, "augment_shift": 3}})
    T = TorchLearner(cfg, "cpu")
    T0 = TorchLearner(ApexConfig.from_dict({"env_conf": env, "Runtime": rt}), "cpu")
    T0.Q.load_state_dict(T.Q.state_dict())
    T0.Q_target.load_state_dict(T.Q_target.state_dict())
    g = torch.Generator().manual_seed(1)
    B = 6
    batch = dict(S_t=torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, generator=g),
                 S_tpn=torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, generator=g),
                 A_t=torch.randint(0, 5, (B,), generator=g), R=torch.rand(B, generator=g) * 3,
                 Gamma=torch.full((B,), 0.97), weights=torch.rand(B, generator=g) + 0.5)
    for u in (0, 5):
        T.num_q_updates = T0.num_q_updates = u
        off = AU.shift_offsets(AU.aug_seed(2), u, 2 * B, 3)
        shifted = dict(batch, S_t=AU.shift_frames(batch["S_t"], off[:B], 3),
                       S_tpn=AU.shift_frames(batch["S_tpn"], off[B:], 3))
        loss, td = T.compute_loss_and_priorities(batch)
        want, td_want = T0.compute_loss_and_priorities(shifted)
        assert torch.equal(T.last_aug_off, off)
        assert torch.equal(loss, want) and torch.equal(td, td_want)
        plain, _ = T0.compute_loss_and_priorities(batch)
        assert not torch.equal(loss, plain)
    out = T.step(batch)
    assert np.isfinite(out["loss"]) and T.num_q_updates == 6
