"""ctypes binding of ``libapex_kernels.so`` (C ABI, built in-tree by ``ops/build.py``).

The library is loaded *after* torch so that its ``libamdhip64.so.7`` NEEDED
entry resolves (by SONAME) to the HIP runtime torch already loaded: kernels
then share torch's device context and run on torch's current stream
(``torch.cuda.current_stream().cuda_stream``), so they are captured by
``torch.cuda.graph`` like any torch op.

On a GPU host a missing or stale library is an error (``require_kernels``),
never a silent fallback: the torch implementations in ``ops/reference.py``
exist only for CPU runs and as test oracles.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import build as _build

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_i64 = ctypes.c_int64
c_u64 = ctypes.c_uint64
c_f = ctypes.c_float


class TreeDesc(ctypes.Structure):
    _fields_ = [("leaf", c_p), ("nodes", c_p), ("off", c_i64 * 8), ("n", c_i64 * 8), ("L", c_i),
                ("min_bits", c_p)]


class RecordDesc(ctypes.Structure):
    _fields_ = [("obs", c_p), ("nxt", c_p), ("act", c_p), ("rew", c_p), ("gam", c_p), ("gen", c_p),
                ("C", c_i), ("cap", c_i64), ("nframes", c_i64)]


class HeadParams(ctypes.Structure):
    _fields_ = [("wv", c_p), ("bv", c_p), ("wa", c_p), ("ba", c_p)]


class HeadLo(ctypes.Structure):
    """Split-mode lo planes of the head's activations / gradient (``HeadLo``, csrc/head_common.h)."""
    _fields_ = [("Hon", c_p), ("Htg", c_p), ("dH", c_p)]


class HeadPart(ctypes.Structure):
    """fc split-K partials consumed by the DDQN head (mirrors ``HeadPart``, csrc/head_common.h)."""
    _fields_ = [("part", c_p), ("zstride", c_i64), ("nz", c_i), ("bias_on", c_p), ("bias_tg", c_p),
                ("two_b", c_i), ("hon", c_p), ("hon_lo", c_p)]


class IsNorm(ctypes.Structure):
    """Batch-max IS normalisation output of the head kernel (``IsNorm``, csrc/head_common.h)."""
    _fields_ = [("wscale", c_p), ("out", c_p), ("valid_count", c_p)]


class HeadIO(ctypes.Structure):
    """What every loss head takes (``HeadIO``, csrc/head_common.h): the first member ``io`` of ``DdqnArgs``,
    ``C51Args``, ``HlgArgs``, ``QRArgs``, ``IqnArgs`` and ``MdqnArgs``."""
    _fields_ = [("Hon", c_p), ("Htg", c_p), ("Pon", HeadParams), ("Ptg", HeadParams), ("act", c_p), ("rew", c_p),
                ("gam", c_p), ("isw", c_p), ("B", c_i), ("A", c_i), ("hidden", c_i), ("grad_scale", c_f),
                ("td_abs", c_p), ("loss", c_p), ("q_out", c_p), ("dH", c_p), ("dhead", c_p), ("zero_ptr", c_p),
                ("zero_n", c_i), ("rescale_eps", c_f), ("lo", HeadLo), ("isn", IsNorm)]


class C51Args(ctypes.Structure):
    """Arguments of the distributional head kernel (``C51Args``, csrc/c51_head.hip)."""
    _fields_ = [("io", HeadIO), ("N", c_i), ("vmin", c_f), ("vmax", c_f)]


class HlgArgs(ctypes.Structure):
    """Arguments of the histogram-loss (HL-Gauss) head kernel (``HlgArgs``, csrc/c51_head.hip)."""
    _fields_ = [("io", HeadIO), ("N", c_i), ("vmin", c_f), ("vmax", c_f), ("sigma_ratio", c_f)]


class QRArgs(ctypes.Structure):
    """Arguments of the quantile-regression head kernel (``QRArgs``, csrc/qr_head.hip)."""
    _fields_ = [("io", HeadIO), ("N", c_i), ("kappa", c_f)]


class IqnEmbed(ctypes.Structure):
    """The cosine embedding of one net (``IqnEmbed``, csrc/iqn_wgrad.h): ``We (2 HS, 64)``, ``be (2 HS,)``."""
    _fields_ = [("w", c_p), ("b", c_p)]


class IqnArgs(ctypes.Structure):
    """Arguments of the implicit quantile head kernel (``IqnArgs``, csrc/iqn_head.hip)."""
    _fields_ = [("io", HeadIO), ("Eon", IqnEmbed), ("Etg", IqnEmbed), ("N", c_i), ("kappa", c_f), ("seed_q", c_u64),
                ("ctr", c_p), ("base", c_p), ("tau_out", c_p), ("dpre", c_p), ("cosT", c_p), ("xg", c_p),
                ("gsum", c_p), ("max_blocks", c_i)]


class IqnWgArgs(ctypes.Structure):
    """Arguments of ``iqn_wgrad_prio_kernel`` (``IqnWgArgs``, csrc/iqn_wgrad.h; launched from csrc/sumtree.hip)."""
    _fields_ = [("dpre", c_p), ("cosT", c_p), ("xg", c_p), ("gsum", c_p), ("act", c_p), ("B", c_i), ("A", c_i),
                ("N", c_i), ("gwv", c_p), ("gbv", c_p), ("gwa", c_p), ("gba", c_p), ("gwtau", c_p), ("gbtau", c_p),
                ("part", c_p)]


class ActorIO(ctypes.Structure):
    """What every actor head takes (``ActorIO``, csrc/head_common.h): the scalar head alone, else first member ``io``."""
    _fields_ = [("H", c_p), ("H_lo", c_p), ("P", HeadParams), ("E", c_i), ("A", c_i), ("hidden", c_i), ("eps", c_p),
                ("seed", c_u64), ("ctr", c_p), ("q_out", c_p), ("a_out", c_p)]


class C51ActorArgs(ctypes.Structure):
    """Arguments of ``c51_actor_head_kernel`` (``C51ActorArgs``, csrc/dist_head.h)."""
    _fields_ = [("io", ActorIO), ("N", c_i), ("vmin", c_f), ("vmax", c_f)]


class QRActorArgs(ctypes.Structure):
    """Arguments of ``qr_actor_head_kernel`` (``QRActorArgs``, csrc/dist_head.h)."""
    _fields_ = [("io", ActorIO), ("N", c_i)]


class IqnActorArgs(ctypes.Structure):
    """Arguments of ``iqn_actor_head_kernel`` (``IqnActorArgs``, csrc/iqn_wgrad.h)."""
    _fields_ = [("io", ActorIO), ("Em", IqnEmbed), ("K", c_i), ("midpoint", c_i), ("seed_q", c_u64), ("tau_ctr", c_p),
                ("stream", c_i), ("tau_out", c_p)]


class MdqnArgs(ctypes.Structure):
    """Arguments of the Munchausen head kernel (``MdqnArgs``, csrc/mdqn_head.hip)."""
    _fields_ = [("io", HeadIO), ("huber", c_i), ("kappa", c_f), ("alpha", c_f), ("tau", c_f), ("clip", c_f),
                ("aux", c_p), ("hp", HeadPart)]


class NoisyNet(ctypes.Structure):
    """One network of a noisy compose launch (``NoisyNet``, csrc/noisy.hip)."""
    _fields_ = [("p", c_p), ("e32", c_p), ("ehi", c_p), ("elo", c_p), ("fc32", c_p), ("xi", c_p)]


class NoisyArgs(ctypes.Structure):
    """Arguments of ``noisy_compose_kernel`` (``NoisyArgs``, csrc/noisy.hip)."""
    _fields_ = [("net", NoisyNet * 2), ("nnets", c_i), ("A", c_i), ("N", c_i), ("stream0", c_i), ("mu", c_i64 * 6),
                ("sg", c_i64 * 6), ("seed", c_u64), ("ctr", c_p), ("base", c_p), ("every", c_i64), ("n_p", c_i64),
                ("n_e", c_i64)]


class NoisyGradArgs(ctypes.Structure):
    """Arguments of ``noisy_sigma_grad_kernel`` (``NoisyGradArgs``, csrc/noisy.hip)."""
    _fields_ = [("g", c_p), ("xi", c_p), ("A", c_i), ("N", c_i), ("mu", c_i64 * 6), ("sg", c_i64 * 6),
                ("n_g", c_i64)]


class AugArgs(ctypes.Structure):
    """Arguments of ``augment_shift_kernel`` (``AugArgs``, csrc/augment.hip)."""
    _fields_ = [("ring", c_p), ("F", c_i64), ("slots", c_p), ("rows", c_i), ("C", c_i), ("pad", c_i), ("seed", c_u64),
                ("ctr", c_p), ("base", c_p), ("out", c_p), ("n_out", c_i64), ("off_out", c_p)]


class ResetRow(ctypes.Structure):
    """One segment of a reset (``ResetRow``, csrc/reset.hip; learner/reset.py ``ResetRow``)."""
    _fields_ = [("start", c_i64), ("end", c_i64), ("period", c_i64), ("live", c_i64), ("bound", c_f), ("alpha", c_f),
                ("const_flag", c_i), ("const_value", c_f)]


class ResetArgs(ctypes.Structure):
    """Arguments of ``reset_perturb_kernel`` (``ResetArgs``, csrc/reset.hip)."""
    _fields_ = [("p", c_p), ("t", c_p), ("v", c_p), ("m", c_p), ("pb", c_p), ("tb", c_p), ("pb_lo", c_p),
                ("tb_lo", c_p), ("n", c_i64), ("seed", c_u64), ("r", c_u64), ("nrows", c_i), ("rows", ResetRow * 32)]


class CfFragOut(ctypes.Structure):
    """The optimizer's stores of the fused forward's online operands (``CfFragOut``,
    csrc/cf_pack.h); all-zero = off."""
    _fields_ = [("w1frag", c_p), ("c2f", c_p), ("w1_off", c_i64), ("w2_off", c_i64), ("C", c_i),
                ("in_scale", c_f), ("c3f", c_p), ("w3_off", c_i64)]


class OptTarget(ctypes.Structure):
    """The soft target an optimizer launch averages (``OptTarget``, csrc/rmsprop_common.h);
    all-zero = off."""
    _fields_ = [("t", c_p), ("tb", c_p), ("tb_lo", c_p), ("rho", c_f), ("tfo", CfFragOut)]


class RmsSegs(ctypes.Structure):
    """Ranges of the flat parameters one optimizer launch updates (``RmsSegs``,
    csrc/sumtree.hip; the sharded data-parallel update)."""
    _fields_ = [("nseg", c_i), ("blk0", c_i * 4), ("off", c_i64 * 3), ("len", c_i64 * 3)]


class OptSched(ctypes.Structure):
    """Update index, lr schedule and Adam constants of an optimizer launch (``OptSched``,
    csrc/rmsprop_common.h); all-zero = RMSprop with the learning rate passed by value."""
    _fields_ = [("ctr", c_p), ("base", c_p), ("adam", c_i), ("warmup", c_i64), ("decay", c_i64),
                ("lr0", ctypes.c_double), ("lr_end", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("t0", c_p)]


class BetaSched(ctypes.Structure):
    """Annealed IS exponent of a draw (``BetaSched``, csrc/sumtree.hip); all-zero = off."""
    _fields_ = [("ubase", c_p), ("beta0", ctypes.c_double), ("beta_end", ctypes.c_double), ("steps", c_i64)]


class RmspropArgs(ctypes.Structure):
    """Everything an optimizer launch takes (``RmspropArgs``, csrc/rmsprop_common.h)."""
    _fields_ = [("p", c_p), ("g", c_p), ("v", c_p), ("m", c_p), ("pb", c_p), ("n", c_i64), ("partials", c_p),
                ("npart", c_i), ("lr", c_f), ("alpha", c_f), ("eps", c_f), ("clip", c_f), ("centered", c_i),
                ("norm_out", c_p), ("pb_lo", c_p), ("wnorm", c_p), ("wn", c_i), ("wstride", c_i), ("fo", CfFragOut),
                ("gpre", c_p), ("npre", c_i64), ("os", OptSched), ("tg", OptTarget)]


class SampleArgs(ctypes.Structure):
    """One stratified draw and where its rows go (``SampleArgs``, csrc/sumtree.hip)."""
    _fields_ = [("t", TreeDesc), ("r", RecordDesc), ("B", c_i), ("seed", c_u64), ("ctr", c_p), ("beta", c_f),
                ("out_idx", c_p), ("out_w", c_p), ("out_gen", c_p), ("out_obs", c_p), ("out_nxt", c_p),
                ("out_act", c_p), ("out_rew", c_p), ("out_gam", c_p), ("out_nxt2", c_p), ("out_obs2", c_p),
                ("shard_stats", c_p), ("shard_rank", c_i), ("shard_world", c_i), ("shard_seed", c_u64),
                ("out_wscale", c_p), ("mcap", c_i64), ("bs", BetaSched)]


class TreeUpdArgs(ctypes.Structure):
    """A priority write-back riding in a weight-gradient launch (``TreeUpdArgs``, csrc/sumtree.hip); the
    launcher fills ``n`` and ``kfirst``."""
    _fields_ = [("t", TreeDesc), ("idx", c_p), ("td", c_p), ("gen_expect", c_p), ("gen", c_p), ("ctr_to_bump", c_p),
                ("alpha", c_f), ("eps", c_f), ("n", c_i), ("kfirst", c_i), ("stats_out", c_p)]


class HeadWgArgs(ctypes.Structure):
    """The head weight gradient's operands (``HeadWgArgs``, csrc/head_common.h)."""
    _fields_ = [("Hon", c_p), ("dhead", c_p), ("B", c_i), ("A", c_i), ("gwv", c_p), ("gbv", c_p), ("gwa", c_p),
                ("gba", c_p), ("HS", c_i), ("Hon_lo", c_p), ("NV", c_i), ("norm_part", c_p)]


class C2dPack(ctypes.Structure):
    """conv2 weight-fragment pack job riding on another launch (``C2dPackJob``, csrc/conv2_wfrag.h)."""
    _fields_ = [("w", c_p), ("w_lo", c_p), ("out", c_p)]


class DdqnArgs(ctypes.Structure):
    """Arguments of the scalar head kernel (``DdqnArgs``, csrc/ddqn_args.h)."""
    _fields_ = [("io", HeadIO), ("huber", c_i), ("kappa", c_f), ("hp", HeadPart), ("pk", C2dPack)]


class ConvDesc(ctypes.Structure):
    """Implicit-GEMM forward/dgrad problem (mirrors ``ConvDesc`` in csrc/conv_mfma.hip)."""
    _fields_ = [("x", c_p), ("frame_slots", c_p), ("w", c_p), ("bias", c_p), ("y", c_p), ("mask", c_p),
                ("N", c_i), ("H", c_i), ("W", c_i), ("Cin", c_i),
                ("OH", c_i), ("OW", c_i), ("Cout", c_i), ("KH", c_i),
                ("KW", c_i), ("stride", c_i), ("pad_h", c_i), ("pad_w", c_i),
                ("mode", c_i), ("relu", c_i), ("ldy", c_i), ("ncls", c_i),
                ("ostride_h", c_i), ("ostride_w", c_i), ("OHfull", c_i), ("OWfull", c_i),
                ("K", c_i), ("in_scale", c_f), ("w_cls_stride", c_i64),
                ("w2", c_p), ("bias2", c_p), ("m_switch", c_i),
                ("bt", c_i), ("ldb", c_i), ("koff", c_i * 16), ("tile_hint", c_i), ("order_hint", c_i),
                ("x_lo", c_p), ("w_lo", c_p), ("w2_lo", c_p), ("y_lo", c_p)]


class WgradDesc(ctypes.Structure):
    """Weight-gradient problem (mirrors ``WgradDesc`` in csrc/conv_mfma.hip)."""
    _fields_ = [("dy", c_p), ("x", c_p), ("frame_slots", c_p), ("slab", c_p), ("bias_slab", c_p),
                ("N", c_i), ("H", c_i), ("W", c_i), ("Cin", c_i),
                ("OH", c_i), ("OW", c_i), ("KH", c_i), ("KW", c_i),
                ("stride", c_i), ("pad_h", c_i), ("pad_w", c_i), ("mode", c_i),
                ("Co", c_i), ("Kc", c_i), ("ldd", c_i), ("ldx", c_i),
                ("rows_per_split", c_i), ("Mred", c_i), ("norm_part", c_p), ("norm_slot0", c_i), ("pad0", c_i),
                ("dy_lo", c_p), ("x_lo", c_p)]


class RedJob(ctypes.Structure):
    """One split-K finalisation job (mirrors ``RedJob`` in csrc/conv_mfma.hip)."""
    _fields_ = [("slab", c_p), ("bslab", c_p), ("out", c_p), ("bout", c_p), ("n", c_i64),
                ("nsplit", c_i), ("nb", c_i), ("s2dC", c_i), ("Kc", c_i), ("scale", c_f), ("blk0", c_i),
                ("cpb", c_i), ("jnorm", c_p)]


class FinalizeDesc(ctypes.Structure):
    """All split-K reductions of a step + squared-norm partials (``FinalizeDesc``)."""
    _fields_ = [("job", RedJob * 4), ("njobs", c_i), ("nrm_n", c_i), ("nrm_ptr", c_p), ("norm_part", c_p),
                ("norm_slot0", c_i), ("nblocks", c_i)]


class Conv1WgDesc(ctypes.Structure):
    """Image-resident conv1 weight gradient (mirrors ``Conv1WgDesc`` in csrc/conv1_wgrad.hip)."""
    _fields_ = [("ring", c_p), ("slots", c_p), ("dy", c_p), ("slab", c_p), ("bias_slab", c_p), ("zero16", c_p),
                ("N", c_i), ("C", c_i), ("dy_lo", c_p), ("wq", c_p)]


class Conv1S2DDesc(ctypes.Structure):
    """conv1 on the space-to-depth ring (mirrors ``Conv1S2DDesc`` in csrc/conv1_s2d.hip)."""
    _fields_ = [("ring", c_p), ("slots", c_p), ("w", c_p), ("w2", c_p), ("bias", c_p), ("bias2", c_p),
                ("y", c_p), ("zero16", c_p), ("scratch", c_p), ("N", c_i), ("C", c_i), ("m_switch", c_i),
                ("in_scale", c_f), ("probe", c_p), ("w32", c_p), ("w2_32", c_p), ("y_lo", c_p),
                ("c2f_src", c_p * 4), ("c2f_out", c_p), ("c2f_bf16", c_i)]


_SIGS = {
    "apex_abi_version": ([], c_i),
    "apex_build_id": ([], ctypes.c_char_p),
    "apex_fill16": ([c_p, c_i64, c_i, c_p], c_i),
    "apex_tree_update": ([TreeDesc, c_p, c_p, c_i, c_i, c_f, c_f, c_p, c_p, c_i, c_p, c_p], c_i),
    "apex_tree_zero_range": ([TreeDesc, c_i64, c_i64, c_p], c_i),
    "apex_replay_insert": ([TreeDesc, RecordDesc, c_i64, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_p],
                           c_i),
    "apex_abi_struct_sizes": ([c_p, c_i], c_i),
    "apex_tree_sample": ([SampleArgs, c_p], c_i),
    "apex_tree_rebuild": ([TreeDesc, c_p], c_i),
    "apex_gather_frames": ([c_p, c_p, c_i, c_i64, c_i64, c_p, c_p], c_i),
    "apex_debug_bounds_enabled": ([], c_i),
    "apex_debug_errors": ([c_p, c_p, c_i], c_i),
    "apex_grad_sqnorm_partials": ([c_p, c_i64, c_p, c_p], c_i),
    "apex_opt_step": ([RmspropArgs, c_p], c_i),
    "apex_cast_bf16": ([c_p, c_p, c_i64, c_p, c_p], c_i),
    "apex_spin_hold": ([c_i, c_i, c_i, c_p, c_p], c_i),
    "apex_grad_finalize": ([FinalizeDesc, c_p], c_i),
    "apex_norm_total": ([c_p, c_i, c_p, c_p], c_i),
    "apex_ddqn_head": ([DdqnArgs, c_p], c_i),
    "apex_value_rescale_probe": ([c_p, c_p, c_p, c_f, c_p, c_i64, c_p], c_i),
    "apex_opt_sample": ([RmspropArgs, SampleArgs, c_p, c_p], c_i),
    "apex_head_wgrad_prio": ([HeadWgArgs, TreeUpdArgs, c_p, c_p, c_p, c_i, c_i, c_p, c_i64, c_p], c_i),
    "apex_fc_wgrad_head_prio": ([WgradDesc, HeadWgArgs, TreeUpdArgs, c_p], c_i),
    "apex_head_wgrad": ([HeadWgArgs, c_p], c_i),
    "apex_c51_head": ([C51Args, c_p], c_i),
    "apex_hlg_head": ([HlgArgs, c_p], c_i),
    "apex_c51_actor_head": ([C51ActorArgs, c_p], c_i),
    "apex_qr_head": ([QRArgs, c_p], c_i),
    "apex_mdqn_head": ([MdqnArgs, c_p], c_i),
    "apex_iqn_head": ([IqnArgs, c_p], c_i),
    "apex_iqn_wgrad": ([IqnWgArgs, c_p], c_i),
    "apex_iqn_wgrad_part_floats": ([], c_i),
    "apex_iqn_wgrad_prio": ([IqnWgArgs, TreeUpdArgs, c_p], c_i),
    "apex_iqn_actor_head": ([IqnActorArgs, c_p], c_i),
    "apex_qr_actor_head": ([QRActorArgs, c_p], c_i),
    "apex_actor_head": ([ActorIO, c_p], c_i),
    "apex_conv1_s2d_fwd": ([Conv1S2DDesc, c_i, c_p], c_i),
    "apex_conv1_wgrad_img": ([Conv1WgDesc, c_i, c_p], c_i),
    "apex_slab_reduce": ([c_p, c_i, c_i64, c_f, c_p, c_p, c_i, c_p, c_i, c_i, c_p], c_i),
    "apex_s2d_pack_w1": ([c_p, c_p, c_i, c_p], c_i),
    "apex_s2d_unpack_w1_grad": ([c_p, c_p, c_i, c_p], c_i),
    "apex_s2d_frames": ([c_p, c_p, c_i64, c_i64, c_i64, c_p], c_i),
    "apex_atari_frames": ([c_p, c_p, c_i64, c_i64, c_i64, c_p], c_i),
    "apex_pack_rows": ([c_p, c_p, c_p, c_i, c_i, c_p, c_i64, c_p], c_i),
    "apex_sqnorm_ranges": ([c_p, c_i64, c_p, c_i64, c_p, c_i, c_p], c_i),
    "apex_copy_segments": ([c_i, c_p, c_p, c_p, c_p], c_i),
    "apex_noisy_xi_len": ([c_i, c_i], c_i),
    "apex_noisy_compose": ([NoisyArgs, c_p], c_i),
    "apex_noisy_sigma_grad": ([NoisyGradArgs, c_p], c_i),
    "apex_augment_shift": ([AugArgs, c_p], c_i),
    "apex_augment_debug_errors": ([c_p, c_p, c_i], c_i),
    "apex_reset_perturb": ([ResetArgs, c_p], c_i),
    "apex_reset_args_size": ([], c_i),
}

_LIB: Optional[ctypes.CDLL] = None
_LOAD_ERROR: Optional[str] = None


def _declare(lib: ctypes.CDLL) -> None:
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            continue
        fn.argtypes = args
        fn.restype = res
    # optional families declared by their own modules (conv / gemm)
    from . import conv_sigs
    conv_sigs.declare(lib)


ABI_VERSION = 19   # csrc/sumtree.hip apex_abi_version(): the launchers' argument lists
SQNORM_PARTIALS = 1024   # what apex_grad_sqnorm_partials writes (csrc/rmsprop_common.h SQNORM_NPART)
# the blocks that cross the ABI by value, in the order of csrc/sumtree.hip apex_abi_struct_sizes()
ABI_STRUCTS = (RmspropArgs, SampleArgs, RmsSegs, TreeUpdArgs, HeadWgArgs, IqnWgArgs, WgradDesc, DdqnArgs, ActorIO,
               C51ActorArgs, QRActorArgs, IqnActorArgs)


def check_struct_sizes(sizes, where: str = "libapex_kernels") -> None:
    """Raise, naming the struct, when the library's ``sizeof`` list differs from the mirrors'."""
    if len(sizes) != len(ABI_STRUCTS):
        raise RuntimeError(f"{where}: {len(sizes)} argument blocks != {len(ABI_STRUCTS)}")
    for cls, size in zip(ABI_STRUCTS, sizes):
        if int(size) != ctypes.sizeof(cls):
            raise RuntimeError(f"{where}: sizeof({cls.__name__}) = {int(size)}, its mirror has {ctypes.sizeof(cls)}")


def load(build_if_missing: bool = True) -> Optional[ctypes.CDLL]:
    """Load the kernel library, after checking the build id compiled into it against
    the tree (ops/build.py: sources, headers, flags, compiler): a stale library is
    rebuilt first (``build_if_missing``) or refused -- never run."""
    global _LIB, _LOAD_ERROR
    if _LIB is not None:
        return _LIB
    debug = debug_bounds_requested()
    try:
        path = _build.ensure_current("kernels_debug" if debug else "kernels", allow_build=build_if_missing)
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        _declare(lib)
        if lib.apex_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{path}: ABI {lib.apex_abi_version()} != {ABI_VERSION}")
        sizes = (c_i * 16)()
        check_struct_sizes(sizes[:lib.apex_abi_struct_sizes(sizes, 16)], path)
        _LIB = lib
    except Exception as e:  # pragma: no cover - depends on toolchain
        _LOAD_ERROR = repr(e)
        _LIB = None
    return _LIB


def debug_bounds_requested() -> bool:
    """``APEX_DEBUG_BOUNDS=1`` selects the bounds-checking kernel library
    (``libapex_kernels_debug.so``, built with ``-DAPEX_DEBUG_BOUNDS``)."""
    return os.environ.get("APEX_DEBUG_BOUNDS", "0") not in ("", "0")


DEBUG_SITES = ("tree_update.leaf", "replay_insert.slot", "tree_sample.slot", "gather_frames.frame",
               "replay_insert.frame_value", "tree_zero_range.slot", "unused6", "unused7")


def debug_errors(reset: bool = True) -> dict:
    """Per-site bounds-violation counts of the debug library (synchronises the
    device).  ``{site: (count, first_bad_index)}`` for sites with violations;
    always empty for the release library."""
    lib = require_kernels()
    counts = (ctypes.c_int * 8)()
    first = (ctypes.c_longlong * 8)()
    check(lib.apex_debug_errors(ctypes.addressof(counts), ctypes.addressof(first), int(reset)), "debug_errors")
    return {DEBUG_SITES[i]: (int(counts[i]), int(first[i])) for i in range(8) if counts[i]}


def available() -> bool:
    return load() is not None


def require_kernels() -> ctypes.CDLL:
    lib = load()
    if lib is None:
        raise RuntimeError(f"apex HIP kernel library unavailable: {_LOAD_ERROR}. "
                           f"Run `python -m apex_dqn_amd.ops.build`.")
    return lib


def stream_ptr(device: Optional[torch.device] = None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def head_lo(Hon_lo=None, Htg_lo=None, dH_lo=None) -> HeadLo:
    """Split-mode lo planes for the head kernels (all None in bf16 mode)."""
    lo = HeadLo()
    lo.Hon, lo.Htg, lo.dH = ptr(Hon_lo), ptr(Htg_lo), ptr(dH_lo)
    return lo


def is_norm(isn=None) -> IsNorm:
    """``isn = (wscale, out[, count])`` of the head ops as the kernels' ``IsNorm`` (all null for None)."""
    s = IsNorm()
    if isn is not None:
        s.wscale, s.out = ptr(isn[0]), ptr(isn[1])
        s.valid_count = ptr(isn[2]) if len(isn) > 2 else None
    return s


def rescale_eps_arg(rescale_eps) -> float:
    """``rescale_eps`` of the head ops as the launchers' float: 0 = off (None), else eps in (0, 1]."""
    if rescale_eps is None:
        return 0.0
    from ..learner.rescale import check_eps
    return check_eps(rescale_eps)


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError {rc}")
