"""Device-side Atari preprocessing (Runtime.atari_preprocess = "device"), the CPU half: the exact
integer arithmetic shared by csrc/atari_frames.hip and its host mirror, the wrapper's raw-frame
mode, the replay's raw append off the HIP path, the config switch and a CPU run of the GPU loop.

Bounds against the fp32 host path (``AtariPreprocess``): its value before rounding differs from
the exact one by fp32 summation error (~1e-4 gray levels at these magnitudes), so the two can
only disagree where the exact value lies that close to a rounding boundary -- by 1, and on at
most 1e-4 of the pixels."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.envs.vector_envs import (RAW_FRAME_SHAPE, AtariPreprocess, AtariPreprocessExact, AtariWrapperVec,
                                           FakeALE, _area_matrix, atari_preprocess_exact, make_vec_env)
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

MAX_DIFF_FRACTION = 1e-4


def _gray(plane: np.ndarray) -> np.ndarray:
    """(210, 160) -> (210, 160, 3) with R = G = B."""
    return np.repeat(plane.astype(np.uint8)[:, :, None], 3, axis=2)


def _check_close_to_host(exact: np.ndarray, host: np.ndarray) -> int:
    d = np.abs(exact.astype(np.int64) - host.astype(np.int64))
    n = int((d != 0).sum())
    print(f"exact vs fp32 host path: {n} of {d.size} pixels differ, max |diff| {int(d.max())}")
    assert d.max() <= 1
    assert n <= MAX_DIFF_FRACTION * d.size
    return n


def test_weights_are_the_integer_area_matrices():
    """The tap formulas the kernel uses equal 5 x / 40 x the host path's area matrices."""
    ry = np.zeros((84, 210))
    for k in range(42):
        ry[2 * k, 5 * k:5 * k + 3] = (2, 2, 1)
        ry[2 * k + 1, 5 * k + 2:5 * k + 5] = (1, 2, 2)
    rx = np.zeros((84, 160))
    for j in range(84):
        for c in range(160):
            rx[j, c] = max(0, min(40 * j + 40, 21 * c + 21) - max(40 * j, 21 * c))
    np.testing.assert_allclose(_area_matrix(84, 210) * 5, ry, atol=1e-9)
    np.testing.assert_allclose(_area_matrix(84, 160) * 40, rx, atol=1e-9)
    assert (ry.sum(1) == 5).all() and (rx.sum(1) == 40).all() and ((rx > 0).sum(1) <= 3).all()
    pre = AtariPreprocessExact()
    np.testing.assert_array_equal(pre.ry, ry)
    np.testing.assert_array_equal(pre.rx, rx)


def test_exact_matches_a_plain_integer_implementation():
    """The float64 matmuls of the mirror against int64 sums written out from the definition."""
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (2,) + RAW_FRAME_SHAPE, dtype=np.uint8)
    m = np.maximum(raw[:, 0], raw[:, 1]).astype(np.int64)
    g = 299 * m[..., 0] + 587 * m[..., 1] + 114 * m[..., 2]              # (2, 210, 160)
    g5 = g.reshape(2, 42, 5, 160)
    rows = np.stack([2 * g5[:, :, 0] + 2 * g5[:, :, 1] + g5[:, :, 2],
                     g5[:, :, 2] + 2 * g5[:, :, 3] + 2 * g5[:, :, 4]], axis=2).reshape(2, 84, 160)
    acc = np.zeros((2, 84, 84), np.int64)
    for j in range(84):
        for c in range(40 * j // 21, min(40 * j // 21 + 3, 160)):
            w = max(0, min(40 * j + 40, 21 * c + 21) - max(40 * j, 21 * c))
            acc[:, :, j] += w * rows[:, :, c]
    q, r = acc // 200000, acc % 200000
    q = q + ((2 * r > 200000) | ((2 * r == 200000) & (q % 2 == 1)))
    np.testing.assert_array_equal(atari_preprocess_exact(raw), q.astype(np.uint8))


def test_ties_round_half_to_even():
    plane = np.zeros((210, 160), np.uint8)
    plane[:, 1] = 20          # output column 0 = (21 * 0 + 19 * 20) / 40 = 9.5 -> 10
    out = atari_preprocess_exact(_gray(plane))
    assert out.shape == (84, 84) and (out[:, 0] == 10).all()
    plane[:, 1] = 60          # 28.5 -> 28
    out = atari_preprocess_exact(_gray(plane))
    assert (out[:, 0] == 28).all()


def test_constant_frames_are_preserved():
    for v in (0, 1, 127, 128, 254, 255):
        f = np.full((210, 160, 3), v, np.uint8)
        assert (atari_preprocess_exact(f) == v).all()
        assert (atari_preprocess_exact(np.stack([f, f])) == v).all()


def test_pair_is_pooled_per_byte_and_shapes():
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, (3,) + RAW_FRAME_SHAPE, dtype=np.uint8)
    out = atari_preprocess_exact(raw)
    assert out.shape == (3, 84, 84) and out.dtype == np.uint8
    np.testing.assert_array_equal(out, atari_preprocess_exact(np.maximum(raw[:, 0], raw[:, 1])))
    np.testing.assert_array_equal(out[1], atari_preprocess_exact(raw[1]))
    # a batch of exactly two pooled frames has to say so
    np.testing.assert_array_equal(atari_preprocess_exact(raw[0], pooled=True),
                                  np.stack([atari_preprocess_exact(raw[0, 0]), atari_preprocess_exact(raw[0, 1])]))
    with pytest.raises(ValueError):
        atari_preprocess_exact(np.zeros((84, 84, 3), np.uint8))


def test_against_fp32_host_path_on_random_pairs():
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 256, (40,) + RAW_FRAME_SHAPE, dtype=np.uint8)
    host = AtariPreprocess()(np.maximum(raw[:, 0], raw[:, 1]))
    _check_close_to_host(atari_preprocess_exact(raw), host)


def test_against_fp32_host_path_on_fake_ale_frames():
    emu = FakeALE(seed=3)
    frames = []
    for t in range(300):
        emu.act(t % 6)
        if emu.game_over():
            emu.reset_game()
        frames.append(emu.getScreenRGB())
    frames = np.stack(frames)
    _check_close_to_host(atari_preprocess_exact(frames), AtariPreprocess()(frames))


def test_wrapper_device_mode_matches_host_mode():
    host = AtariWrapperVec([FakeALE(seed=i) for i in range(3)], seed=4)
    dev = AtariWrapperVec([FakeALE(seed=i) for i in range(3)], seed=4, preprocess="device")
    assert not host.raw_frames and dev.raw_frames and dev.raw_shape == RAW_FRAME_SHAPE == (2, 210, 160, 3)
    assert dev.obs_shape == host.obs_shape == (84, 84) and dev.frame_out
    fh, fd = host.reset(), dev.reset()
    assert fd.shape == (3,) + RAW_FRAME_SHAPE and fd.dtype == np.uint8
    np.testing.assert_array_equal(fd[:, 0], fd[:, 1])           # one frame exists after a reset
    hs, ds = [fh], [atari_preprocess_exact(fd)]
    rng = np.random.default_rng(0)
    life_lost = game_over = pair_differs = False
    for _ in range(60):
        act = rng.integers(0, 6, 3)
        buf = np.full((3,) + RAW_FRAME_SHAPE, 7, np.uint8)
        fh, rh, dh, ih = host.step(act)
        fd, rd, dd, idv = dev.step(act, out=buf)
        assert fd is buf
        np.testing.assert_array_equal(rh, rd)
        np.testing.assert_array_equal(dh, dd)
        assert set(ih) == set(idv)
        for k in ih:
            np.testing.assert_array_equal(ih[k], idv[k])
        for e in np.nonzero(ih["real_done"])[0]:                 # first frame after a game over
            np.testing.assert_array_equal(fd[e, 0], fd[e, 1])
        life_lost |= bool((dh & ~ih["real_done"]).any())
        game_over |= bool(ih["real_done"].any())
        pair_differs |= bool((fd[:, 0] != fd[:, 1]).any())
        hs.append(fh)
        ds.append(atari_preprocess_exact(fd))
    assert life_lost and game_over and pair_differs
    _check_close_to_host(np.stack(ds), np.stack(hs))
    # without out= a fresh array of the raw shape comes back
    fd2 = dev.step(np.zeros(3, np.int64))[0]
    assert fd2.shape == (3,) + RAW_FRAME_SHAPE and fd2.dtype == np.uint8


def test_wrapper_raw_pair_is_the_last_two_frames_of_the_skip():
    dev = AtariWrapperVec([FakeALE(seed=0)], noop_max=0, episodic_life=False, preprocess="device")
    dev.reset()
    twin = FakeALE(seed=0)
    twin.reset_game()
    frames = []
    for _ in range(4):
        twin.act(dev.actions[2])
        frames.append(twin.getScreenRGB())
    raw = dev.step([2])[0]
    np.testing.assert_array_equal(raw[0, 0], frames[2])
    np.testing.assert_array_equal(raw[0, 1], frames[3])


def test_factory_and_wrapper_reject_bad_modes():
    env = make_vec_env("fake_ale", "PongNoFrameskip-v4", 2, 6, seed=1, preprocess="device")
    assert env.raw_frames and env.reset().shape == (2,) + RAW_FRAME_SHAPE
    assert not make_vec_env("fake_ale", "PongNoFrameskip-v4", 2, 6, seed=1).raw_frames
    for backend in ("synthetic", "cartpole"):
        with pytest.raises(ValueError):
            make_vec_env(backend, "x", 2, 2, preprocess="device")
    with pytest.raises(ValueError):
        make_vec_env("fake_ale", "x", 2, 6, preprocess="gpu")
    with pytest.raises(ValueError):
        AtariWrapperVec([FakeALE()], preprocess="gpu")


def test_replay_append_raw_frames_on_cpu_equals_mirror_then_append():
    a = GpuReplayShard(16, 16, 5, 2, device=torch.device("cpu"))
    b = GpuReplayShard(16, 16, 5, 2, device=torch.device("cpu"))
    rng = np.random.default_rng(2)
    for _ in range(3):                                           # 6 frames through a ring of 5: one wrap
        raw = rng.integers(0, 256, (2,) + RAW_FRAME_SHAPE, dtype=np.uint8)
        sa = a.append_raw_frames(raw)
        sb = b.append_frames(atari_preprocess_exact(raw))
        np.testing.assert_array_equal(sa, sb)
        assert a.frame_head == b.frame_head
        assert torch.equal(a.frames, b.frames)
    slots = torch.tensor([[0, 1], [2, 3], [4, 0]], dtype=torch.int32)
    assert torch.equal(a.gather_frames(slots), b.gather_frames(slots))
    np.testing.assert_array_equal(a.gather_frames(slots)[2, 1].numpy(), atari_preprocess_exact(raw)[1])
    assert a.stage_frames(2, raw=True) is None                   # pinned staging is a GPU-shard thing
    with pytest.raises(ValueError):
        a.append_raw_frames(np.zeros((2, 84, 84), np.uint8))
    c = GpuReplayShard(16, 16, 5, 2, frame_shape=(42, 42), device=torch.device("cpu"))
    with pytest.raises(ValueError):
        c.append_raw_frames(raw)


def _cfg(**runtime):
    return {"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "PongNoFrameskip-v4"},
            "Actor": {"num_actors": 6, "n_step_transition_batch_size": 6, "Q_network_sync_freq": 5},
            "Learner": {"min_replay_mem_size": 40, "replay_sample_size": 8, "remove_old_xp_freq": 4,
                        "q_target_sync_freq": 5},
            "Replay_Memory": {"soft_capacity": 120},
            "Runtime": dict({"replay_capacity": 150, "log_every": 4, "use_graphs": False}, **runtime)}


def test_config_switch():
    assert ApexConfig().Runtime.atari_preprocess == "host"
    assert ApexConfig.from_dict(_cfg(env_backend="fake_ale")).Runtime.atari_preprocess == "host"
    for backend in ("fake_ale", "fake_ale_target", "ale"):
        cfg = ApexConfig.from_dict(_cfg(env_backend=backend, atari_preprocess="device"))
        assert cfg.Runtime.atari_preprocess == "device"
    for backend in ("synthetic", "cartpole"):
        with pytest.raises(ValueError):
            ApexConfig.from_dict(_cfg(env_backend=backend, atari_preprocess="device"))
    with pytest.raises(ValueError):
        ApexConfig.from_dict(_cfg(env_backend="fake_ale", atari_preprocess="gpu"))
    bad = _cfg(env_backend="fake_ale", atari_preprocess="device", network="impala")
    bad["env_conf"]["state_shape"] = [4, 64, 64]
    with pytest.raises(ValueError):
        ApexConfig.from_dict(bad)


def test_gpu_loop_on_cpu_with_device_preprocessing():
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict(_cfg(env_backend="fake_ale", atari_preprocess="device"))
    out = train_frames(cfg, "cpu", 8)
    assert out["learner"].num_q_updates == 8
    assert out["actors"].env.raw_frames
    assert out["losses"] and np.isfinite(out["losses"]).all()
    assert out["actors"].inserted > 0 and out["replay"].size() > 0
    assert int(out["replay"].frames.max()) > 0                   # preprocessed frames reached the ring
