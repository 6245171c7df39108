"""Kernel-path switches: ONE registry.

Every alternative kernel path that survived as an A/B knob lives here with its
measured winner as the default (the measurements are cited per field; the history is
in docs/PERF_NOTES.md).  Production code reads ``SW.<name>``; tests flip a path with
``monkeypatch.setattr(SW, name, value)``; experiments override from the environment
with ONE variable::

    APEX_SWITCHES="conv2_img=0,wg_rows3=384" python bench.py

``bench.py`` prints every non-default value in its JSON (``switches``), so a number
measured off the defaults is labelled as such.
"""
from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass
from typing import Any, Dict


@dataclass
class Switches:
    # conv2 forward on the image-resident kernel (csrc/conv2_img.hip) instead of the generic
    # implicit GEMM (bf16 learner without the fused conv1 -> conv2 kernel, actors)
    conv2_img: bool = True
    # split conv2 forward: weights packed into per-lane fragment order by the launcher
    # (76.2 -> 71.0 us at 1536 images, profiles/r2_split_conv2_packed_fwd.jsonl)
    c2f_pack: bool = True
    # conv1 -> conv2 forward fused with y1 in LDS (csrc/conv12_fused.hip), split mode
    conv12_fused: bool = True
    # conv3 fused into the conv1 -> conv2 kernel (y2 read from LDS; csrc/conv12_fused.hip) for
    # launches of at most this many images (0: never).  With its weights in coalesced C3F
    # fragments (written by the optimizer) and its biases loaded ahead, the fused conv3 takes
    # ~3.7 k cycles per image and wins at every size: 512 rows 2,733-2,740 vs 2,678-2,692
    # fp32 updates/s (bf16 4,523-4,529 vs 4,433-4,451), emulated W = 8 157.1-157.3 vs
    # 163.1-169.7 us, W = 4 192.7-193.5 vs 198.1-202.9 us (profiles/r6_ab_conv123_fused_c3f.txt;
    # with the weights read from OHWI rows it lost at 512 rows, r6_ab_conv123_fused.txt)
    conv123_max_images: int = 1 << 20
    # with conv3 fused, the forward writes y2 to memory only for the S_t rows (the backward's
    # input; csrc/conv12_fused.hip Conv12Desc::y2_n): the 2B rows of S_t+n keep it in LDS, 21 MB
    # of stores per 512-row fp32 update that nothing read.  The step's results are the same
    # bytes.  conv12_fused_kernel in the 512-row fp32 step 118.4 -> 114.8 us
    # (profiles/pr33_step_timeline_fp32_parent.txt, pr33_step_timeline_fp32_conv3_wgrad_img.txt);
    # parent / this tree / this tree with the switch off, 4 interleaved runs each at 20 / 5
    # steps: 2,928-2,956 / 2,974-3,015 / 2,912-2,927 updates/s (profiles/pr33_ab_switches.txt).
    # The 200 / 20 comparison has not been taken
    conv12_y2_rows: bool = True
    # the fused forward's one-plane variant for the bf16 learner (4,105 vs 3,790 steps/s,
    # profiles/r3_ab_conv12_bf16_fused_4105_vs_3790.txt)
    conv12_bf16: bool = True
    # image-resident conv3 / conv2 data gradients (csrc/conv2_img.hip)
    conv3_dgrad_img: bool = True
    conv2_dgrad_img: bool = True
    # split-mode conv3 data gradient on the image-resident kernel
    # (csrc/conv3_dgrad_img_split.hip, the same bits as the generic implicit GEMM) for batches
    # of at least conv3_dgrad_img_split_min images.  Isolated, 7 interleaved repeats of 50
    # launches: 13.5-14.2 vs 21.0-21.9 us at 512 images, 8.9-9.5 vs 12.0-12.7 at 256, 8.3-8.6
    # vs 10.2-10.6 at 146, 7.9-8.0 vs 9.9-10.1 at 74 (profiles/pr6_conv3_dgrad_isolated.txt).
    # Inside the 512-row fp32 step 13.5 vs 22.8 us, and conv21_bwd_fused starts 18.5 instead of
    # 27.4 us after it; 5 interleaved runs each of the parent and this tree: 2,928-2,967
    # (median 2,950) vs 2,884-2,910 (2,894) updates/s at 200 / 20 steps, 2,932-2,967 (2,943) vs
    # 2,876-2,917 (2,890) at 20 / 5 (profiles/pr6_ab_conv3_dgrad_img.txt).  Emulated rank
    # steps, forced on vs off, 3 runs each: W = 8 (74 rows) 154.0-154.9 vs 158.6-161.1 us, W = 4
    # (146 rows) 190.3-191.5 vs 192.3-195.6.  The threshold is the smallest size measured;
    # below 74 images nobody has measured, so those keep the generic kernel
    conv3_dgrad_img_split: bool = True
    conv3_dgrad_img_split_min: int = 74
    # split conv2 data gradient: one workgroup per (image, stride-parity class) up to this
    # many images (0: never), per image above it
    conv2_dgrad_cls_max: int = 256
    # conv2's data gradient and conv1's weight gradient in one per-image kernel, dY1 in LDS
    # only (csrc/conv21_bwd_fused.hip): split mode, 4 frames, static order, batches above
    # conv2_dgrad_cls_max; on or off the step's results are the same bits.  Isolated at 512
    # images 44.9 us vs 38.2 + 25.2 for the pair; the 512-row fp32 step, 5 interleaved runs
    # each: 2,838-2,862 (median 2,843) vs 2,696-2,716 (2,699) updates/s at 200 / 20 steps,
    # 2,819-2,836 (2,826) vs 2,669-2,715 (2,683) at 20 / 5 (profiles/pr2_ab_conv21_bwd_fused.txt)
    conv21_bwd_fused: bool = True
    # the optimizer + sample launch stores the fused forward's online weight fragments
    # (+0.5-1 %, profiles/r3_ab_optimizer_frag_stores_*.txt)
    opt_frags: bool = True
    # the fc layer's split-K epilogue runs inside the DDQN head launch
    fc_epi_in_head: bool = True
    # single-rank step: the weight gradients (fc + heads + priority write-back, conv3,
    # conv2) on a second stream beside the data-gradient chain (graph branches)
    bwd_branches: bool = True
    # the GPU actors' fc forward: this K split (0: the chip-filling split of the learner)
    actor_fc_ksplit: int = 4
    # single-rank branched backward: the fc weight gradient (+ head wgrad + priorities) on
    # the main stream right after the fc dgrad, the branch forking after it ("on"), on the
    # branch beside the dgrad chain ("off"), "auto": main for fp32-class at >= 256 rows
    fc_wgrad_main: str = "auto"
    # cap on the fc forward's K splits (0: fill the chip, ops/fused_ops.py fc_fwd); the DDQN
    # head sums the splits' partials (the deferred epilogue)
    fc_ksplit_max: int = 0
    # device-side image work queues in the persistent kernels: "auto" = only where RCCL's
    # kernels may hold CUs (the DP conv backward at world > 1), "on" / "off" force them
    work_queue: str = "auto"
    # split-K reduction rows per workgroup of the conv3 / conv2 weight gradients (0: the
    # tuned defaults in ops/conv.py)
    wg_rows3: int = 0
    wg_rows2: int = 0
    # split-mode conv2 weight gradient on the row-resident kernel (csrc/conv2_wgrad_rows.hip:
    # every y1 input row staged once per (split, kernel row) workgroup, the same bits as the
    # generic kernel) for batches of at least conv2_wgrad_rows_min images.  Its grid is half
    # the generic kernel's, so it pays only where the generic one needs two rounds: isolated
    # at 512 images 28.8-30.6 vs 29.9-32.1 us (a tie), at 256 images 27.5-28.5 vs 16.6-17.3,
    # at 74 images 15.5-15.9 vs 9.5-9.7 (profiles/pr4_conv2_wgrad_isolated.txt).  Inside the
    # 512-row fp32 step, where it ends the backward on the branch, 58.2 vs 61.9 us; 5
    # interleaved runs each of the parent and this tree: 2,838-2,855 (median 2,850) vs
    # 2,805-2,827 (2,814) updates/s at 200 / 20 steps, 2,815-2,845 (2,843) vs 2,796-2,813
    # (2,803) at 20 / 5 (profiles/pr4_ab_conv2_wgrad_rows.txt).  The threshold is the one
    # size the step was measured at; between 279 images (where the generic grid passes 256
    # blocks) and 511 nobody has measured
    conv2_wgrad_rows: bool = True
    conv2_wgrad_rows_min: int = 512
    # split-mode conv3 weight gradient on the image-resident kernel (csrc/conv3_wgrad_img.hip:
    # dY3 and y2 staged once per image, the whole 64 x 576 gradient in the registers of
    # conv3_wgrad_img_grid persistent workgroups, one slab plane each) for batches of at
    # least conv3_wgrad_img_min images.  OFF: correct (tests/test_gpu_conv3_wgrad_img.py) but
    # slower than the generic kernel at every size measured.  Isolated, 7 interleaved repeats
    # of 50 launches, kernel (+ its grad_finalize): generic 13.4-13.7 (+ 3.4) us at 512 images;
    # 64 workgroups 25.7-26.5 (+ 3.4), 128: 18.7-18.9 (+ 3.9), 256: 15.5-15.6 (+ 8.0); at 256
    # images 12.6 vs 14.4 (128) / 13.0 (256), at 146 images 8.6 vs 14.1, at 74 images 8.0 vs
    # 12.7 (profiles/pr33_conv3_wgrad_isolated.txt): ~1.7 us per image and workgroup, as
    # modelled, on top of ~12 us per launch that the model did not have.  In the 512-row fp32
    # step 24.1 us against the generic kernel's 18.0; on vs off in one tree, 4 interleaved
    # runs each at 20 / 5 steps: 2,832-2,858 vs 2,912-2,927 updates/s (grid 128, the best of
    # 64 / 128 / 256; profiles/pr33_ab_switches.txt); emulated W = 8 rank step 154.0-158.0 vs
    # 150.7-153.2 us (profiles/pr33_emulated_ranks.txt).  docs/PERF_NOTES.md has the account.
    # The threshold is the one size at which the step was worth asking about
    conv3_wgrad_img: bool = False
    conv3_wgrad_img_min: int = 512
    conv3_wgrad_img_grid: int = 128
    # IMPALA weight gradients: workgroups per conv and the partial-slab cap (floats)
    impala_wg_target: int = 512
    impala_slab_cap: int = 8 << 20
    # IMPALA bf16 fused residual block rows per band at 16 ch x 42 (swept: 21 777, 14 786, 11 778)
    resblock_r16: int = 14
    # IMPALA stack 1: the max-pool backward inside the ring conv's weight-gradient staging
    impala_pool_wgrad: bool = True
    # IMPALA split kernels' launch shapes "key=value;..." ('' = the defaults of
    # ops/impala.py _split_bands): rb<C>x<H>=R (residual block rows), sc<cin>x<cout>x<H>p<pool>=R
    # (conv rows), wg<cin>x<cout>x<H>=R/threads (weight-gradient variant), wt<cin>x<cout>x<H>=N
    # (weight-gradient workgroup target)
    isplit_bands: str = ""
    # DP step (learner/dp_step.py): the sharded update's fc weight gradient on the branch
    # right behind the factor exchange (True) or on main after conv1's weight gradient
    # (False: emulated W = 8 160.5-162.1 vs 178.6-180.7 us, W = 4 201.5-202.0 vs
    # 199.7-203.6 -- the branch becomes the critical chain; profiles/r6_ab_dp_switches.txt)
    dp_fc_shard_branch: bool = False
    # DP step: one main-stream event for the branch's conv3 + conv2 weight gradients (one
    # cross-queue edge fewer on the critical path; with the fused conv3: emulated W = 4
    # 195.0 / 195.1 vs 197.2 / 197.6 us, W = 8 164.1 / 163.2 vs 170.0 / 166.2,
    # profiles/r6_ab_misc.txt)
    dp_branch_one_wait: bool = True
    # DP step, sharded update with the factored exchange: this rank's fc weight-gradient rows
    # as split-K partials of this many reduction rows each, reduced in conv1's finalize
    # launch (0: one launch over all rows writing the gradient itself; -1: 256 at 8+ ranks,
    # else 128 -- emulated W = 8 157.3 vs 159.0 us, W = 4 193.9 vs 190.5 at 256,
    # profiles/r6_ab_dp_fc_split_rows.txt)
    dp_fc_split_rows: int = -1
    # DP step, sharded update: the [w2, wfc) bucket's clip-norm partials on the branch and
    # conv1's bucket summed inside the optimizer launch (no norm launch on main; emulated W =
    # 8 with the fc gradient on main: 160.5-162.1 us vs 166-169 before)
    dp_norm_split: bool = True

    @classmethod
    def from_env(cls, spec: str = None) -> "Switches":
        sw = cls()
        spec = os.environ.get("APEX_SWITCHES", "") if spec is None else spec
        for item in spec.split(","):
            item = item.strip()
            if not item:
                continue
            if "=" not in item:
                raise ValueError(f"APEX_SWITCHES item must be name=value, got {item!r}")
            k, v = item.split("=", 1)
            f = {f.name: f for f in dataclasses.fields(cls)}.get(k)
            if f is None:
                raise ValueError(f"unknown kernel switch {k!r}")
            setattr(sw, k, _parse(f.type, v))
        return sw

    def non_default(self) -> Dict[str, Any]:
        d = Switches()
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)
                if getattr(self, f.name) != getattr(d, f.name)}


def _parse(typ, v: str):
    t = typ if isinstance(typ, str) else typ.__name__
    if t == "bool":
        return v.lower() not in ("0", "false", "off", "no")
    if t == "int":
        return int(v)
    return v


SW = Switches.from_env()
