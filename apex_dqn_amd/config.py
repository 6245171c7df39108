"""Typed configuration for the Ape-X engine.

Accepts the reference ``parameters.json`` schema verbatim (four sections:
``env_conf``, ``Actor``, ``Learner``, ``Replay_Memory`` --
reference ``parameters.json:1-34``, consumed at ``main.py:29-33``) and adds an
optional ``Runtime`` section for everything the reference hard-codes
(learner T at ``main.py:46``, optimizer at ``learner.py:26``, the
ExperienceBuffer gamma at ``actor.py:25``) or lacks entirely (device, world
size, checkpointing, network variant, env backend).

``--set Section.key=value`` overrides are parsed with JSON semantics
(``--set Learner.replay_sample_size=512``,
``--set env_conf.state_shape=[4,84,84]``).
"""
from __future__ import annotations

import copy
import dataclasses
import json
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np


@dataclass
class EnvConf:
    state_shape: List[int] = field(default_factory=lambda: [1, 84, 84])
    action_dim: int = 4
    name: str = "RiverraidNoFrameskip-v4"


@dataclass
class ActorConf:
    num_actors: int = 5
    T: int = 50000
    num_steps: int = 3
    epsilon: float = 0.4
    alpha: float = 7.0
    gamma: float = 0.99
    n_step_transition_batch_size: int = 5
    Q_network_sync_freq: int = 500


@dataclass
class LearnerConf:
    remove_old_xp_freq: int = 100
    q_target_sync_freq: int = 2500
    min_replay_mem_size: int = 20000
    replay_sample_size: int = 32
    load_saved_state: Any = False


@dataclass
class ReplayConf:
    soft_capacity: int = 100000
    priority_exponent: float = 0.6
    importance_sampling_exponent: float = 0.4


@dataclass
class RuntimeConf:
    """Extension section (not present in the reference; all optional)."""

    device: str = "auto"            # "auto" | "cpu" | "cuda"
    world_size: int = 1
    dtype: str = "fp32"             # GPU learner precision: "fp32" (the reference's; split hi/lo bf16
                                    # operands, 3 MFMAs per product) | "bf16" (bf16 operands)
    seed: int = 0
    learner_T: int = 500000         # reference hard-codes 500000 (main.py:46)
    network: str = "auto"           # "auto" | "nature64" | "nature32" | "mlp" | "impala"
    env_backend: str = "auto"       # "auto" | "synthetic" | "cartpole" | "ale" | "fake_ale" | "fake_ale_target"
    frame_stack: Optional[int] = None  # defaults to state_shape[0]
    actors_per_rank: Optional[int] = None  # defaults to num_actors / world_size
    obs_scale: float = 1.0 / 255.0  # uint8 -> float scale fed to conv nets
    # optimizer: centered RMSprop as in the Ape-X paper (reference passes the
    # decay 0.95 as weight_decay by mistake, learner.py:26).
    lr: float = 0.00025 / 4
    rms_decay: float = 0.95
    rms_eps: float = 1.5e-7
    centered_rmsprop: bool = True
    optimizer: str = "rmsprop"      # "rmsprop" (above) | "adam" (same launches, csrc/rmsprop_common.h OPT_ADAM;
                                    # reuses the RMSprop state buffers, bias-corrected with t = update index + 1)
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1.5e-4
    # lr(u), u = updates completed before the current one, evaluated on the device (learner/schedules.py):
    # lr (u + 1) / warmup while u < lr_warmup_steps, then a linear ramp from lr to lr_end over lr_decay_steps
    lr_warmup_steps: int = 0
    lr_decay_steps: int = 0
    lr_end: Optional[float] = None
    # IS exponent annealed from Replay_Memory.importance_sampling_exponent to is_beta_end over
    # is_beta_anneal_steps updates: the batch of update u carries beta(u)
    is_beta_end: Optional[float] = None
    is_beta_anneal_steps: int = 0
    grad_clip: float = 40.0
    loss: str = "huber"             # "huber" | "mse" (0.5*delta^2, reference learner.py:48)
    huber_delta: float = 1.0
    # distributional (C51) dueling head: num_atoms >= 2 atoms on the support [v_min, v_max]; the loss is the
    # cross-entropy against the projected n-step target distribution (loss / huber_delta do not apply), the
    # priority stays |E[target] - E[q]| (learner/losses.py c51_loss).  1 = the scalar head.  Single-rank
    # NatureCNN (csrc/c51_head.hip) and the torch learners (mlp); not IMPALA, the DP step or the graph learner
    num_atoms: int = 1
    v_min: float = -10.0
    v_max: float = 10.0
    # the distributional head's kind, read only when num_atoms >= 2: "categorical" (C51, above) or "quantile"
    # (QR-DQN, csrc/qr_head.hip): num_atoms quantiles per action at tau_i = (2 i + 1) / (2 N), the quantile Huber
    # loss with kappa = huber_delta (> 0; loss does not apply), no support (v_min / v_max are ignored), the same
    # priority and the same refusals (learner/losses.py quantile_huber_loss)
    dist_head: str = "categorical"
    # "implicit" (IQN, csrc/iqn_head.hip): num_atoms = N tau samples per state in the loss (N and N' of the paper),
    # the head at the scalar head's shapes gated by a 64-cosine embedding of tau after the fc layer; the quantile
    # head's loss with sampled fractions (learner/losses.py iqn_loss, learner/iqn.py the draws' mirror).
    # iqn_actor_samples = K: the samples behind the actors' and the greedy evaluation's q
    iqn_actor_samples: int = 32
    # "hl_gauss" (the Gaussian histogram loss, Imani & White 2018 / Farebrother et al. 2024; csrc/c51_head.hip
    # hlg_head_kernel): the categorical head, its support, weights, checkpoint keys and actor head, trained against
    # the scalar double-DQN target spread over the bins as a Gaussian of sigma = hl_gauss_sigma_ratio bin widths
    # (finite, > 0; the paper's 0.75) instead of the projected target distribution; the priority is |y - q| against
    # that scalar target (learner/losses.py hl_gauss_loss).  loss / huber_delta do not apply; C51's refusals
    hl_gauss_sigma_ratio: float = 0.75
    # factorised NoisyNet fc and head layers (Fortunato et al. 2018; learner/noisy.py, csrc/noisy.hip): the two
    # stream layers and the two heads carry W = mu + sigma * (xi_out (x) xi_in), one draw per update for the online
    # net and one for the target net, one per noisy_actor_resample batched inference calls for an actor group;
    # sigma starts at noisy_sigma0 / sqrt(fan-in).  Single-rank NatureCNN with any head kind and the torch
    # learners (mlp); not IMPALA, the DP step or the graph learner.  The epsilon ladder is not touched
    noisy: bool = False
    noisy_sigma0: float = 0.5
    noisy_actor_resample: int = 1
    # Munchausen-DQN target for the scalar head (Vieillard et al. 2020; learner/losses.py munchausen_loss,
    # csrc/mdqn_head.hip): T = R + alpha clamp(tau ln pi(a | Q_target(S_t)), clip, 0) + Gamma * the target net's
    # soft value at S_t+n, pi = softmax(Q_target / tau); no online argmax.  The forward runs the online net on
    # S_t only and the target net on S_t+n and S_t.  Single-rank NatureCNN and the torch learners (mlp), with or
    # without Runtime.noisy; not the distributional heads, IMPALA, the DP step or the graph learner
    munchausen: bool = False
    munchausen_alpha: float = 0.9
    munchausen_tau: float = 0.03
    munchausen_clip: float = -1.0
    # soft (Polyak) target network: after every update t <- (1 - rho) t + rho p over the whole flat parameter
    # vector, inside the optimizer launch (csrc/rmsprop_common.h EMA, learner/schedules.py target_ema the mirror).
    # 0 = the hard copy every Learner.q_target_sync_freq updates; > 0 turns that copy off (the key is ignored).
    # Single-rank NatureCNN with any head kind and the torch learners (mlp); not IMPALA, the DP step or the
    # graph learner
    target_ema_rate: float = 0.0
    # invertible value rescaling of the n-step target (Pohlen et al. 2018; learner/rescale.py, csrc/value_rescale.h):
    # the network learns h(Q), h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x, against T = h(R + Gamma h^-1(Q_target)),
    # so returns of any magnitude are learnable without clipping the rewards.  All four loss heads (per target
    # sample on the quantile heads, the support in transformed space on the categorical one) and the actors'
    # initial priorities; q_values and the actor heads return transformed q.  Single-rank NatureCNN and the torch
    # learners (mlp), with noisy layers, Adam, the schedules and the soft target; not Runtime.munchausen, IMPALA,
    # the DP step or the graph learner
    value_rescale: bool = False
    value_rescale_eps: float = 1e-3
    # random-shift (DrQ) augmentation of the sampled frames (Kostrikov et al. 2020; learner/augment.py,
    # csrc/augment.hip): every sampled S_t and S_t+n is padded by augment_shift pixels with edge replication and
    # cropped back to 84 x 84 at an offset drawn per (sample, state, update), at the head of every update inside the
    # captured step.  0 = off (the launches and the bits of before), at most 8.  Single-rank NatureCNN with every
    # head kind, noisy layers, the Munchausen target, Adam, the schedules, the soft target and value rescaling, and
    # the torch learner on 84 x 84 stacks; not IMPALA, the DP step or the graph learner.  Actors and evaluation
    # see the frames as they are
    augment_shift: int = 0
    # periodic shrink-and-perturb resets (Nikishin et al. 2022; SR-SPR, D'Oro et al. 2023; BBF, Schwarzer et al.
    # 2023; learner/reset.py, csrc/reset.hip): after every update whose count is a positive multiple of
    # reset_interval every parameter becomes alpha * old + (1 - alpha) * a fresh draw from its layer's initial
    # distribution -- alpha = reset_shrink_encoder for the conv layers, reset_shrink_head for everything behind
    # them -- in both nets with the same draw, the optimizer moments are zeroed and Adam's step count restarts; the
    # replay carries the knowledge across.  0 = off (no buffer, no launch, the launches and the bits of before).
    # Single-rank NatureCNN with every head kind, noisy layers, the Munchausen target, value rescaling, the random
    # shift, Adam, the schedules and either target, and the torch learners (mlp); not IMPALA, the DP step or the
    # graph learner
    reset_interval: int = 0
    reset_shrink_encoder: float = 0.5
    reset_shrink_head: float = 0.0
    # Atari wrappers clip rewards to {-1, 0, +1} (envs/vector_envs.py AtariWrapperVec); false keeps the raw rewards
    # (with value_rescale; the two keys are independent)
    clip_rewards: bool = True
    priority_eps: float = 1e-6      # priority floor: leaves hold (|delta| + priority_eps)^alpha
    use_is_weights: bool = True
    is_normalise: str = "batch_max"  # IS weights (N P(i))^-beta divided by their max over the sampled batch
                                    # ("batch_max", the PER / Ape-X papers' 1 / max_i w_i; with DP the global
                                    # batch) or over the whole replay ("global_min": (p / p_min)^-beta, which
                                    # shrinks every update when a few priorities sit at the floor)
    ckpt_dir: Optional[str] = None
    ckpt_freq: int = 0              # learner steps between checkpoints (0 = off)
    metrics_path: Optional[str] = None
    log_every: int = 100
    param_publish_freq: int = 1     # learner steps between param publishes to actors
    use_hip_kernels: bool = True    # GPU path: hand-written HIP kernels
    use_graphs: bool = True         # GPU path: capture the learner step in a HIP graph
    profile_phases: bool = False    # at every log interval, time one eager step per phase (CUDA events)
    episode_lines_per_log: int = 4  # reference-format episode console lines per log interval (rank 0)
    torch_profile_dir: Optional[str] = None  # torch.profiler (ROCm activities) trace of a few steps
    torch_profile_start: int = 50   # first profiled learner step
    torch_profile_steps: int = 5
    resume: bool = True             # continue from ckpt_dir/checkpoint.pt when it exists (restarts)
    allreduce_dtype: str = "fp32"   # DP gradient all-reduce payload: "fp32" (exact) | "bf16" (half the bytes)
    presample: bool = True          # draw step t+1's batch at the end of step t (fused learner; on the HIP
                                    # backend inside the optimizer launch)
    graph_steps: int = 20           # learner updates per HIP-graph launch in learner.steps(n) (single
                                    # rank and DP alike: the DP step's collectives are captured too;
                                    # divides the default eviction cadence; 20 vs 10: 2,732 / 2,726 vs
                                    # 2,703 / 2,684 steps/s at 20 / 5, 2,729 / 2,744 vs 2,718 / 2,717 at
                                    # 200 / 20, profiles/r6_ab_graph_steps.txt; 10 vs 4: 3505 vs 3472)
    actor_learner_ratio: float = 0.0  # in-process actor steps per learner step (0 = separate)
    replay_capacity: Optional[int] = None  # physical capacity, global over the ranks' shards
                                           # (default: soft_capacity * 1.25 + 1024)
    heartbeat_timeout: float = 60.0
    comm_backend: str = "native"    # DP collectives: "native" (parallel/rccl.py: own RCCL communicator on its
                                    # own comm stream; the step is one captured HIP graph) | "torch"
                                    # (torch.distributed process group; eager DP steps: its watchdog's
                                    # event cache is not capture-safe on this ROCm / torch build)
    force_dp: bool = False          # run the data-parallel step (collectives + sharded replay) even at
                                    # world 1 (needs an initialised process group; checks / overhead)
    batch_scope: str = "global"     # DP: "global" = Learner.replay_sample_size is the batch of ONE update
                                    # summed over all ranks (the reference's / Ape-X's update, learner.py:68:
                                    # strong scaling; each rank computes the rows of the global draw that fall
                                    # in its shard) | "per_rank" = every rank draws up to that many rows (a
                                    # W-rank update averages up to W x the batch: weak scaling)
    dp_batch_slack: float = 0.125   # global scope: rows a rank can hold beyond B/W, as a fraction of B/W (plus
                                    # 2): the draw takes exactly B strata while no shard holds more than
                                    # (rows - 2) / B of the total priority mass, fewer otherwise
    dp_fc_exchange: str = "auto"    # DP exchange of the fc layer's gradient: "allreduce" (the 1024 x 3136 fp32
                                    # gradient) | "factors" (all-gather every rank's dH / fc-input rows -- the
                                    # operands the kernels use -- and form the gradient of the whole global
                                    # batch on each rank: ~(B_total x 4160) values instead of 3.2 M, exact and
                                    # bit-identical across ranks) | "auto" (factors while 1 < W and W x rows
                                    # <= 1024)
    dp_rows_adaptive: bool = True   # global scope: grow the per-rank rows (and recapture the step) when a
                                    # shard's share of the priority mass outgrows them, checked at init and
                                    # at every eviction (learner/dp_step.py _fit_rows), so M stays B
    dp_shard_update: str = "auto"   # DP: the fc layer's optimizer (96 % of the parameters) sharded by output rows
                                    # over the ranks, the updated rows all-gathered (learner/dp_step.py):
                                    # "on" | "off" | "auto" (on at world > 1 when 1024 / (64 W) is whole)
    replica_check_every: int = 5000  # DP: learner steps between replica checksum checks (0 = off)
    step_timeout: float = 300.0     # GPU loop watchdog: seconds a queued learner chunk may take
    async_actors: bool = True       # GPU loop: the actor group steps on its own host thread
    actor_precision: str = "learner"  # GPU actor inference: "learner" (the learner's precision; fp32-class
                                      # split kernels with dtype fp32, as the reference's fp32 actors) |
                                      # "bf16" (hi planes only: faster, bf16-class q-values / priorities)
    actor_graph: bool = True        # GPU actors: the inference launches replayed as one HIP graph per step
                                    # (host launch overhead: ~0.13 ms per step for the eager launches)
    actor_pipeline: int = 2         # async GPU actors: the rank's envs as this many groups stepped in
                                    # turn, so one group's host env step overlaps another's inference
                                    # (actors/gpu_actor.py PipelinedActorGroups; 1 = one group)
    atari_preprocess: str = "host"  # emulator-backed envs (ale / fake_ale / fake_ale_target) on the GPU loop:
                                    # "host" (fp32 numpy max / gray / area resize in the actor's host thread,
                                    # the 84x84 frame goes H2D) | "device" (the two raw 210x160x3 frames go H2D
                                    # and one kernel, csrc/atari_frames.hip, preprocesses them into the frame
                                    # ring in exact integer arithmetic; 84x84 states only)
    learner_stream_priority: bool = True   # async GPU actors: learner on a high-priority HIP stream
                                    # (runtime/actor_thread.py), concurrent with the learner


@dataclass
class ApexConfig:
    env_conf: EnvConf = field(default_factory=EnvConf)
    Actor: ActorConf = field(default_factory=ActorConf)
    Learner: LearnerConf = field(default_factory=LearnerConf)
    Replay_Memory: ReplayConf = field(default_factory=ReplayConf)
    Runtime: RuntimeConf = field(default_factory=RuntimeConf)

    # ------------------------------------------------------------------ io
    @classmethod
    def from_dict(cls, d: Dict[str, Any], strict: bool = False) -> "ApexConfig":
        sections = {
            "env_conf": EnvConf,
            "Actor": ActorConf,
            "Learner": LearnerConf,
            "Replay_Memory": ReplayConf,
            "Runtime": RuntimeConf,
        }
        kw = {}
        for name, klass in sections.items():
            raw = dict(d.get(name, {}) or {})
            known = {f.name for f in dataclasses.fields(klass)}
            unknown = set(raw) - known
            if unknown and strict:
                raise KeyError(f"unknown keys in section {name}: {sorted(unknown)}")
            kw[name] = klass(**{k: v for k, v in raw.items() if k in known})
        extra = set(d) - set(sections)
        if extra and strict:
            raise KeyError(f"unknown sections: {sorted(extra)}")
        cfg = cls(**kw)
        cfg.validate()
        return cfg

    @classmethod
    def load(cls, path: str, overrides: Sequence[str] = ()) -> "ApexConfig":
        with open(path, "r") as f:
            d = json.load(f)
        d = apply_overrides(d, overrides)
        return cls.from_dict(d)

    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2)

    # ------------------------------------------------------------ derived
    def validate(self) -> None:
        ss = self.env_conf.state_shape
        if not isinstance(ss, (list, tuple)) or len(ss) not in (1, 3):
            raise ValueError(f"env_conf.state_shape must be [C,H,W] or [D], got {ss}")
        if self.env_conf.action_dim < 1:
            raise ValueError("env_conf.action_dim must be >= 1")
        if self.Actor.num_actors < 1:
            raise ValueError("Actor.num_actors must be >= 1")
        if self.Actor.num_steps < 1:
            raise ValueError("Actor.num_steps must be >= 1")
        if not (0.0 <= self.Actor.gamma <= 1.0):
            raise ValueError("Actor.gamma must be in [0,1]")
        if self.Learner.replay_sample_size < 1:
            raise ValueError("Learner.replay_sample_size must be >= 1")
        if self.Runtime.world_size < 1:
            raise ValueError("Runtime.world_size must be >= 1")
        if self.Runtime.comm_backend not in ("torch", "native"):
            raise ValueError("Runtime.comm_backend must be 'torch' or 'native'")
        if int(self.Runtime.actor_pipeline) < 1:
            raise ValueError("Runtime.actor_pipeline must be >= 1")
        if self.Runtime.actor_precision not in ("learner", "bf16"):
            raise ValueError("Runtime.actor_precision must be 'learner' or 'bf16'")
        if self.Runtime.is_normalise not in ("batch_max", "global_min"):
            raise ValueError("Runtime.is_normalise must be 'batch_max' or 'global_min'")
        if self.Runtime.batch_scope not in ("global", "per_rank"):
            raise ValueError("Runtime.batch_scope must be 'global' or 'per_rank'")
        if not self.Runtime.dp_batch_slack >= 0.0:
            raise ValueError("Runtime.dp_batch_slack must be >= 0")
        if self.Runtime.dp_shard_update not in ("auto", "on", "off"):
            raise ValueError("Runtime.dp_shard_update must be 'auto', 'on' or 'off'")
        if self.Runtime.dp_fc_exchange not in ("auto", "factors", "allreduce"):
            raise ValueError("Runtime.dp_fc_exchange must be 'auto', 'factors' or 'allreduce'")
        if self.Runtime.atari_preprocess not in ("host", "device"):
            raise ValueError("Runtime.atari_preprocess must be 'host' or 'device'")
        if self.Runtime.atari_preprocess == "device":
            if self.env_backend not in ("ale", "fake_ale", "fake_ale_target"):
                raise ValueError(f"Runtime.atari_preprocess='device' needs an env backend with raw Atari frames "
                                 f"(ale, fake_ale, fake_ale_target), got {self.env_backend!r}")
            if len(ss) != 3 or tuple(ss[1:]) != (84, 84):
                raise ValueError(f"Runtime.atari_preprocess='device' produces 84x84 frames, got state_shape {ss}")
        if self.Runtime.loss not in ("huber", "mse"):
            raise ValueError("Runtime.loss must be 'huber' or 'mse'")
        rt = self.Runtime
        if rt.optimizer not in ("rmsprop", "adam"):
            raise ValueError(f"Runtime.optimizer must be 'rmsprop' or 'adam', got {rt.optimizer!r}")
        if int(rt.lr_warmup_steps) < 0 or int(rt.lr_decay_steps) < 0 or int(rt.is_beta_anneal_steps) < 0:
            raise ValueError("Runtime.lr_warmup_steps, lr_decay_steps and is_beta_anneal_steps must be >= 0")
        if (rt.lr_end is not None) != (int(rt.lr_decay_steps) > 0):
            raise ValueError("Runtime.lr_end and Runtime.lr_decay_steps > 0 need each other")
        if (rt.is_beta_end is not None) != (int(rt.is_beta_anneal_steps) > 0):
            raise ValueError("Runtime.is_beta_end and Runtime.is_beta_anneal_steps > 0 need each other")
        if rt.is_beta_end is not None and not rt.use_is_weights:
            raise ValueError("Runtime.is_beta_end anneals the IS weights: it needs Runtime.use_is_weights")
        net = self.network
        na = rt.num_atoms
        if isinstance(na, bool) or not isinstance(na, int) or not (na == 1 or 2 <= na <= 64):
            raise ValueError(f"Runtime.num_atoms must be 1 or an integer in [2, 64] (one lane per atom), got {na!r}")
        if not float(rt.v_min) < float(rt.v_max):
            raise ValueError(f"Runtime.v_min must be below Runtime.v_max, got {rt.v_min} / {rt.v_max}")
        if rt.dist_head not in ("categorical", "quantile", "implicit", "hl_gauss"):
            raise ValueError(f"Runtime.dist_head must be 'categorical', 'quantile', 'implicit' or 'hl_gauss', got "
                             f"{rt.dist_head!r}")
        sr = rt.hl_gauss_sigma_ratio
        if na >= 2 and rt.dist_head == "hl_gauss" and (
                isinstance(sr, bool) or not isinstance(sr, (int, float)) or not 0.0 < float(sr) < float("inf")):
            raise ValueError(f"Runtime.hl_gauss_sigma_ratio (the histogram loss's sigma in bin widths) must be a "
                             f"finite number > 0, got {sr!r}")
        ks = rt.iqn_actor_samples
        if isinstance(ks, bool) or not isinstance(ks, int) or not 1 <= ks <= 64:
            raise ValueError(f"Runtime.iqn_actor_samples must be an integer in [1, 64] (one lane per sample), got {ks!r}")
        if na == 1 and rt.dist_head != "categorical":
            raise ValueError(f"Runtime.dist_head={rt.dist_head!r} needs Runtime.num_atoms >= 2 (the scalar head has "
                             f"no distribution)")
        if na >= 2 and rt.dist_head in ("quantile", "implicit") and not float(rt.huber_delta) > 0.0:
            raise ValueError(f"Runtime.dist_head={rt.dist_head!r} needs Runtime.huber_delta > 0 (the quantile Huber "
                             f"loss's kappa), got {rt.huber_delta}")
        if na >= 2 and rt.dist_head == "implicit":
            if rt.noisy is True:
                raise ValueError("Runtime.noisy with Runtime.dist_head='implicit' is not built: the noisy layers "
                                 "compose the categorical and quantile heads only")
            if rt.munchausen is True:
                raise ValueError("Runtime.munchausen with Runtime.dist_head='implicit' (M-IQN) is not built: the "
                                 "Munchausen target is the scalar head's")
        if na >= 2:
            if net not in ("nature64", "nature32", "mlp"):
                raise ValueError(f"Runtime.num_atoms={na} needs network nature64, nature32 or mlp, got {net!r}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError(f"Runtime.num_atoms={na} runs on a single rank: the data-parallel step "
                                 f"(world_size > 1, force_dp) has no distributional head")
        if not isinstance(rt.noisy, bool):
            raise ValueError(f"Runtime.noisy must be true or false, got {rt.noisy!r}")
        if not float(rt.noisy_sigma0) > 0.0:
            raise ValueError(f"Runtime.noisy_sigma0 (Runtime.noisy's initial sigma scale) must be > 0, got "
                             f"{rt.noisy_sigma0}")
        nr = rt.noisy_actor_resample
        if isinstance(nr, bool) or not isinstance(nr, int) or nr < 1:
            raise ValueError(f"Runtime.noisy_actor_resample (Runtime.noisy's inference calls per actor draw) must "
                             f"be an integer >= 1, got {nr!r}")
        if rt.noisy:
            if net not in ("nature64", "nature32", "mlp"):
                raise ValueError(f"Runtime.noisy needs network nature64, nature32 or mlp, got {net!r}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError("Runtime.noisy runs on a single rank: the data-parallel step (world_size > 1, "
                                 "force_dp) has no noisy layers")
        if not isinstance(rt.munchausen, bool):
            raise ValueError(f"Runtime.munchausen must be true or false, got {rt.munchausen!r}")
        if not 0.0 <= float(rt.munchausen_alpha) <= 1.0:
            raise ValueError(f"Runtime.munchausen_alpha (the bonus scale) must be in [0, 1], got "
                             f"{rt.munchausen_alpha}")
        if not float(rt.munchausen_tau) > 0.0:
            raise ValueError(f"Runtime.munchausen_tau (the softmax temperature) must be > 0, got "
                             f"{rt.munchausen_tau}")
        if not float(rt.munchausen_clip) < 0.0:
            raise ValueError(f"Runtime.munchausen_clip (the lower clip of tau ln pi) must be < 0, got "
                             f"{rt.munchausen_clip}")
        if rt.munchausen:
            if na >= 2:
                raise ValueError(f"Runtime.munchausen is a target of the scalar head: Runtime.num_atoms={na} "
                                 f"(a distributional head) is not supported")
            if net not in ("nature64", "nature32", "mlp"):
                raise ValueError(f"Runtime.munchausen needs network nature64, nature32 or mlp, got {net!r}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError("Runtime.munchausen runs on a single rank: the data-parallel step (world_size > 1, "
                                 "force_dp) has no Munchausen target")
        rho = rt.target_ema_rate
        if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not 0.0 <= float(rho) <= 1.0:
            raise ValueError(f"Runtime.target_ema_rate (the soft target's rate) must be a number in [0, 1], got "
                             f"{rho!r}")
        if float(rho) > 0.0:
            if net not in ("nature64", "nature32", "mlp"):
                raise ValueError(f"Runtime.target_ema_rate needs network nature64, nature32 or mlp, got {net!r}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError("Runtime.target_ema_rate runs on a single rank: the data-parallel step "
                                 "(world_size > 1, force_dp) keeps the hard target sync")
        for key in ("value_rescale", "clip_rewards"):
            if not isinstance(getattr(rt, key), bool):
                raise ValueError(f"Runtime.{key} must be true or false, got {getattr(rt, key)!r}")
        eps = rt.value_rescale_eps
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 < float(eps) <= 1.0:
            raise ValueError(f"Runtime.value_rescale_eps (the linear term of h) must be a number in (0, 1], got {eps!r}")
        if rt.value_rescale:
            if rt.munchausen:
                raise ValueError("Runtime.value_rescale with Runtime.munchausen is not built: the Munchausen target "
                                 "is not rescaled")
            if net not in ("nature64", "nature32", "mlp"):
                raise ValueError(f"Runtime.value_rescale needs network nature64, nature32 or mlp, got {net!r}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError("Runtime.value_rescale runs on a single rank: the data-parallel step (world_size > 1, "
                                 "force_dp) has no rescaled target")
        P = rt.augment_shift
        if isinstance(P, bool) or not isinstance(P, int) or not 0 <= P <= 8:
            raise ValueError(f"Runtime.augment_shift (the random shift's pad in pixels) must be an integer in [0, 8], "
                             f"got {P!r}")
        if P >= 1:
            if net == "impala":
                raise ValueError("Runtime.augment_shift: the IMPALA step has no frame augmentation (it is the "
                                 "NatureCNN learner's)")
            if net not in ("nature64", "nature32"):
                raise ValueError(f"Runtime.augment_shift needs network nature64 or nature32, got {net!r}")
            if len(ss) != 3 or tuple(ss[1:]) != (84, 84):
                raise ValueError(f"Runtime.augment_shift shifts 84x84 frames, got state_shape {ss}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError("Runtime.augment_shift runs on a single rank: the data-parallel step (world_size > 1, "
                                 "force_dp) has no frame augmentation")
        ri = rt.reset_interval
        if isinstance(ri, bool) or not isinstance(ri, int) or ri < 0:
            raise ValueError(f"Runtime.reset_interval (updates between shrink-and-perturb resets, 0 = off) must be an "
                             f"integer >= 0, got {ri!r}")
        for key in ("reset_shrink_encoder", "reset_shrink_head"):
            al = getattr(rt, key)
            if isinstance(al, bool) or not isinstance(al, (int, float)) or not 0.0 <= float(al) <= 1.0:
                raise ValueError(f"Runtime.{key} (the share of the old value a reset keeps) must be a number in "
                                 f"[0, 1], got {al!r}")
        if ri > 0:
            if net == "impala":
                raise ValueError("Runtime.reset_interval: the IMPALA step has no periodic resets (they are the "
                                 "NatureCNN learner's)")
            if net not in ("nature64", "nature32", "mlp"):
                raise ValueError(f"Runtime.reset_interval needs network nature64, nature32 or mlp, got {net!r}")
            if int(rt.world_size) > 1 or rt.force_dp:
                raise ValueError("Runtime.reset_interval runs on a single rank: the data-parallel step (world_size > 1, "
                                 "force_dp) has no periodic resets")
        if net in ("nature64", "nature32", "impala") and len(ss) != 3:
            raise ValueError(f"network {net} needs an image state_shape [C,H,W], got {ss}")
        if net in ("nature64", "nature32") and tuple(ss[1:]) != (84, 84):
            raise ValueError(f"NatureCNN expects 84x84 frames, got {ss}")

    @property
    def network(self) -> str:
        if self.Runtime.network != "auto":
            return self.Runtime.network
        return "nature64" if len(self.env_conf.state_shape) == 3 else "mlp"

    @property
    def distributional(self) -> bool:
        return int(self.Runtime.num_atoms) >= 2

    def head_kw(self) -> Dict[str, Any]:
        """The dueling modules' head arguments (models/dueling.py)."""
        rt = self.Runtime
        kw = dict(num_atoms=int(rt.num_atoms), v_min=float(rt.v_min), v_max=float(rt.v_max),
                  dist_head=str(rt.dist_head))
        if self.implicit:  # (only then: the other heads' call is the one of before)
            kw.update(iqn_actor_samples=int(rt.iqn_actor_samples))
        if rt.noisy:       # (only then: the non-noisy call is the one of before)
            kw.update(noisy=True, noisy_sigma0=float(rt.noisy_sigma0))
        return kw

    @property
    def rescale_eps(self) -> Optional[float]:
        """eps of the rescaled target (learner/rescale.py), or None with ``Runtime.value_rescale`` off: the
        ``rescale_eps`` of the loss oracles and the head ops."""
        return float(self.Runtime.value_rescale_eps) if self.Runtime.value_rescale else None

    def munchausen_kw(self) -> Dict[str, float]:
        """(alpha, tau, clip) of the Munchausen target (learner/losses.py munchausen_loss)."""
        rt = self.Runtime
        return dict(alpha=float(rt.munchausen_alpha), tau=float(rt.munchausen_tau), clip=float(rt.munchausen_clip))

    @property
    def quantile(self) -> bool:
        """The distributional head is the quantile-regression one (Runtime.dist_head)."""
        return self.distributional and self.Runtime.dist_head == "quantile"

    @property
    def hl_gauss(self) -> bool:
        """The categorical head is trained with the histogram loss (Runtime.dist_head)."""
        return self.distributional and self.Runtime.dist_head == "hl_gauss"

    @property
    def implicit(self) -> bool:
        """The distributional head is the implicit quantile one (Runtime.dist_head)."""
        return self.distributional and self.Runtime.dist_head == "implicit"

    @property
    def env_backend(self) -> str:
        if self.Runtime.env_backend != "auto":
            return self.Runtime.env_backend
        name = self.env_conf.name.lower()
        if "cartpole" in name:
            return "cartpole"
        if "synthetic" in name:
            return "synthetic"
        # Atari ids: use ALE when importable, otherwise a synthetic env of the same shape
        try:  # pragma: no cover - ale_py is not installed in this image
            import ale_py  # noqa: F401
            return "ale"
        except Exception:
            return "synthetic"

    @property
    def frame_stack(self) -> int:
        if self.Runtime.frame_stack is not None:
            return int(self.Runtime.frame_stack)
        ss = self.env_conf.state_shape
        return int(ss[0]) if len(ss) == 3 else 1

    @property
    def replay_capacity(self) -> int:
        if self.Runtime.replay_capacity is not None:
            return int(self.Runtime.replay_capacity)
        return int(self.Replay_Memory.soft_capacity * 1.25) + 1024

    def shard_capacity(self, world: int) -> Tuple[int, int]:
        """(soft, physical) transitions held by ONE of ``world`` replay shards: the
        global FIFO bound ``Replay_Memory.soft_capacity`` (``replay.py:71-80``) split
        evenly, ceil-rounded; the physical ring keeps the configured headroom."""
        w = max(int(world), 1)
        soft = -(-int(self.Replay_Memory.soft_capacity) // w)
        if self.Runtime.replay_capacity is not None:
            phys = -(-int(self.Runtime.replay_capacity) // w)
        else:
            phys = int(soft * 1.25) + 1024
        return soft, max(phys, soft)

    def dp_batch(self, world: int, dp: bool = True) -> Tuple[int, int]:
        """(rows per rank, cap on the global batch M) of a learner update on ``world``
        data-parallel ranks (``dp``: the sharded DP step runs, world > 1 or forced).

        * no DP: (B, B);
        * ``batch_scope = "per_rank"``: (B, W B) -- every rank draws up to B rows;
        * ``batch_scope = "global"``: one update takes B = ``replay_sample_size`` draws
          over all shards, as the reference's single learner (``learner.py:68``); rank r
          holds ceil(B / W (1 + dp_batch_slack)) + 2 rows (B at W = 1), enough for its
          share of the global draw while its shard carries at most (rows - 2) / B of
          the total mass (replay/gpu_replay.py ``enable_sharding``)."""
        B = int(self.Learner.replay_sample_size)
        W = max(int(world), 1)
        if not dp:
            return B, B
        if self.Runtime.batch_scope == "per_rank":
            return B, W * B
        if W == 1:
            return B, B
        rows = int(np.ceil(B / W * (1.0 + float(self.Runtime.dp_batch_slack)) - 1e-9)) + 2
        return min(rows, B + 2), B

    def copy(self) -> "ApexConfig":
        return copy.deepcopy(self)


def _parse_value(v: str) -> Any:
    try:
        return json.loads(v)
    except (json.JSONDecodeError, ValueError):
        low = v.lower()
        if low in ("true", "false"):
            return low == "true"
        return v


def apply_overrides(d: Dict[str, Any], overrides: Sequence[str]) -> Dict[str, Any]:
    """Apply ``Section.key=value`` overrides to a raw config dict."""
    d = copy.deepcopy(d)
    for ov in overrides or ():
        if "=" not in ov:
            raise ValueError(f"override must be Section.key=value, got {ov!r}")
        path, val = ov.split("=", 1)
        parts = path.split(".")
        if len(parts) != 2:
            raise ValueError(f"override path must be Section.key, got {path!r}")
        sec, key = parts
        d.setdefault(sec, {})[key] = _parse_value(val)
    return d


def epsilon_ladder(num_actors: int, epsilon: float = 0.4, alpha: float = 7.0) -> List[float]:
    """Per-actor exploration rates eps_i = eps^(1 + alpha*i/(N-1)).

    Reference ``actor.py:111-114`` divides by zero for N=1 (defect A13); a
    single actor gets the base epsilon here.
    """
    denom = max(num_actors - 1, 1)
    return [float(epsilon ** (1.0 + alpha * i / denom)) for i in range(num_actors)]
