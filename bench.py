#!/usr/bin/env python3
"""bench.py -- the driver's benchmark contract for the CoDA hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload sa|model] [--full] [--dump-outputs DIR]

A "step" is one forward+backward pass of the hot path over one batch of 8
synthetic SUN-RGBD-shaped scenes (20 000 points) per GPU, inputs resident in HBM
before the timed region.  Prints ONE JSON line on rank 0 (see the task contract):
scenes/s over all ranks, plus

A plain run measures the headline and nothing else: set-up, warm-up (with the settle blocks and the host-slack probe
below), the K timed steps, the outputs of the last one if --dump-outputs is given, the line.  Everything else the
line can carry is measured only with --full: the extra steps that time the other kernels (``roofline_others``, the
whole-backward figures of ``roofline``), the unchanged caller's leg (``value_unchanged``), the ball query alone and at
B = 64, the collectives timed alone (``comm``), the extra configurations and the CPU baseline.

* ``roofline``     model workload: the dominant kernel of the step's critical path, the
                   encoder self-attention dK/dV kernel (fp32 MFMA bound): its flops per
                   launch (SURVEY.md 8d attention-core counts) / its average launch
                   duration, measured live with HIP events on the launch stream inside
                   the timed region (coda_mha_timing_*).  sa workload: the
                   ball_query(+group) operator against HBM (3 126 016 B/scene).
* ``roofline_others`` the other attention kernels (timed in extra steps right after the
                   timed region) and the ball_query(+group) operator (BASELINE.json's
                   "ball_query HBM GB/s"), same definitions.
* ``cpu_baseline`` the CPU oracle port (C ops + torch-CPU layers) on the host
                   cores, bounded sample, rank 0 at N=1 only.

CODA_BENCH_DRY=1 runs this file's control flow on the CPU with a toy module (tests/test_bench_dry.py).

Multi-GPU: one process per GPU (torch.distributed, backend "nccl" = RCCL); scenes
shard data-parallel (weak scaling, 8 scenes per GPU); the only exchange is the
DDP gradient all-reduce (+ SyncBatchNorm statistics), as in the reference
(main.py:993-996).
"""
import argparse
import contextlib
import gc
import json
import math
import os
import re
import sys
import time

T_PROCESS_START = time.perf_counter()  # (value_unchanged's two readings carry their time since process start)

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from coda_neurips2023_amd.pointnet2 import _ext, pointnet2_modules  # noqa: E402
from coda_neurips2023_amd.synthetic_scenes import make_batch  # noqa: E402

B_PER_GPU = 8
N_POINTS = 20000
M_CENTRES = 2048
NSAMPLE = 64
RADIUS = 0.2
# ball_query 12N+12M+4MS, group (C=3) 4MS+12N+12MS, per scene
BQ_GROUP_BYTES_PER_SCENE = (12 * N_POINTS + 12 * M_CENTRES + 4 * M_CENTRES * NSAMPLE) + \
                           (4 * M_CENTRES * NSAMPLE + 12 * N_POINTS + 12 * M_CENTRES * NSAMPLE)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
BQ_TRAFFIC_PMC = int((1089.0 * 2 + 3012.2 + 2666.0 * 2 + 16384.0) * 1024)  # profiles/r05_pmc_ball_query.md, B = 8
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 matrix peak (v_mfma_f32_32x32x16_bf16)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense fp32 matrix peak (v_mfma_f32_32x32x2_f32)
# MFMA flops of one attention kernel per (query, key, model-channel) triple: forward QK^T + PV;
# dK/dV kernel S = QK^T (recomputed), dP = dO V^T, dV = P^T dO, dK = dS^T Q; dQ kernel S, dP, dQ = dS K.
# SURVEY.md 8d counts the whole backward as 8 (+4 "if recomputed") = the dV, dK, dP, dQ products plus
# one recomputation; the two-kernel split executes 14.
# dqg: dQ = dS K alone (dS from the dK/dV kernel's workspace); bwdf: the decoder cross-attention's one-kernel backward
# (S, dP, dV, dK, dQ partial tiles: 10); dqr / delta: its partial-tile sum and rowsum(dO * O) -- no MFMA flops, their time counts
ATTN_FLOPS = {"fwd": 4, "dkv": 8, "dq": 6, "dqg": 2, "bwdf": 10, "dqr": 0, "delta": 0, "ktp": 0}
# of those, the units SURVEY 8d's ALGORITHMIC count credits (backward = 8: dV, dP, dK, dQ; recomputing S is extra work)
ATTN_FLOPS_ALG = {"fwd": 4, "dkv": 6, "dq": 2, "dqg": 2, "bwdf": 8, "dqr": 0, "delta": 0, "ktp": 0}
ATTN_UNITS_NOTE = {"fwd": "4 algorithmic (QK^T, PV)",
                   "dkv": "6 algorithmic (dP, dV, dK) + 2 recomputed (S = QK^T)",
                   "dq": "2 algorithmic (dQ = dS K) + 4 recomputed (S, dP)",
                   "dqg": "2 algorithmic (dQ = dS K, dS read from the dK/dV kernel's workspace)",
                   "bwdf": "8 algorithmic (dP, dV, dK, dQ) + 2 recomputed (S = QK^T), one kernel",
                   "dqr": "no MFMA work: the key blocks' partial dQ tiles summed in fixed order"}
# HBM bytes per launch of the 2048x2048 dK/dV kernel from PMC: FETCH_SIZE 55 374 KB x 2 (gfx950 correction) +
# WRITE_SIZE 49 272 KB, separate rocprofv3 --pmc passes (profiles/r01_pmc_attention_hbm.md); algorithmic 101.2 MB
# HBM bytes per launch of the encoder's dK/dV kernel from PMC passes (FETCH_SIZE x2 + WRITE_SIZE): with the dS workspace
# route of round 4 (the kernel also streams dS = 8 x 4 x 2048 x 2048 floats = 537 MB out) / the two-kernel form of round 3
ATTN_DKV_TRAFFIC_DS = int(45656.3 * 2 * 1024) + int(565421.8 * 1024)  # profiles/r06_pmc_attention_hbm.md (r05: 44360.2 / 565560.2); algorithmic: 84 MB in + 570 MB out
ATTN_DKV_TRAFFIC = 94_247_117 + 45_362_074      # profiles/r03_pmc_attention_hbm.md


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--workload", default="auto", choices=["auto", "sa", "model", "model40k"])
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-extras", action="store_true",
                   help="skip the extra single-GPU configurations (configs[1] set abstraction, configs[4] share: "
                        "40k points / 512 queries / bf16 attention) that follow the headline measurement")
    p.add_argument("--prefetch", choices=["on", "off"], default="on",
                   help="model workload: sample (FPS) batch i+1 on a side stream during step i")
    p.add_argument("--full", action="store_true",
                   help="after the headline also run every secondary measurement (other kernels, the unchanged caller, "
                        "collectives, extra configurations, CPU baseline); off: the headline alone")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step computed to DIR/<name>.npy (rank 0; the step starts from the "
                        "state after the warm-up, so equal arguments give equal inputs)")
    return p.parse_args()


# --dump-outputs: while this is a dict, every step function stores in it what its step computed (the loss, the loss
# terms, the predictions); the timed loop runs with it set and the last step's entries are what gets written
_capture = None


def build_dry_workload(dev):
    """CODA_BENCH_DRY=1 (tests/test_bench_dry.py): a toy torch module on the CPU in place of the detector, so
    that THIS FILE's control flow -- warm-up, barriers, timed loop, max over ranks, the steps after the timed
    region, one JSON line from rank 0 -- can be exercised with several gloo ranks on a machine without GPUs.
    It measures nothing and takes the same branches as the model workload."""
    torch.manual_seed(0)
    mod = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.BatchNorm1d(16), torch.nn.ReLU(),
                              torch.nn.Linear(16, 1)).to(dev).train()

    def step(model, batch, pre_encoded=None, with_dict=False):
        if dist.is_initialized():  # stands in for the SyncBatchNorm statistics exchange of the forward pass
            dist.all_reduce(torch.ones(32))
        out = model(batch["point_clouds"].reshape(-1, 3))
        loss = out.square().mean()
        if _capture is not None:
            _capture.update(loss=loss, outputs={"toy": out})
        return (loss, {"loss_toy": loss.detach(), "loss_toy_0": loss.detach() * 2}) if with_dict else loss

    return mod, step, "dry run of bench.py's control flow (toy CPU module, no kernels, numbers meaningless)", "dry"


def build_workload(kind, dev):
    """Returns (module, step_fn(model, batch) -> loss, description, kind)."""
    if os.environ.get("CODA_BENCH_DRY") == "1":
        return build_dry_workload(dev)
    if kind in ("auto", "model"):
        return build_model_workload(dev)
    if kind == "model40k":  # profiling aid: the configs[4] share as the main workload (bf16 attention, 512 queries)
        return build_model_workload(dev, nq=512, config_tag="configs[4], one GPU's share", attn="bf16")
    torch.manual_seed(0)
    mod = pointnet2_modules.PointnetSAModuleVotes(radius=RADIUS, nsample=NSAMPLE, npoint=M_CENTRES,
                                                  mlp=[0, 64, 128, 256], normalize_xyz=True).to(dev)
    mod.train()

    def step(model, batch):
        new_xyz, feat, inds = model(batch["point_clouds"])
        loss = feat.square().mean()
        if _capture is not None:
            _capture.update(loss=loss, outputs={"new_xyz": new_xyz, "features": feat, "inds": inds})
        return loss

    desc = ("configs[1]: PointNet++ SA (FPS 20000->2048 + ball_query r=0.2 nsample=64 + group + "
            "SharedMLP[3,64,128,256]+BN+ReLU + max-pool) fwd+bwd, batch=8/GPU, fp32")
    return mod, step, desc, "sa"


def recipe_args(nq, **model_overrides):
    """scripts/coda_sunrgbd_stage2.sh on top of main.py's defaults (main.py:154-205): the matcher costs and the
    loss weights of the recipe BASELINE.json's configs quote (both alignment terms live)."""
    from coda_neurips2023_amd.criterion import _WEIGHT_ARGS
    from coda_neurips2023_amd.model_3detr import default_args
    ns = default_args(nqueries=nq, **model_overrides)
    for attr in _WEIGHT_ARGS.values():
        setattr(ns, attr, 0)
    for k, v in dict(loss_no_object_weight=0.05, loss_angle_cls_weight=0.1, loss_angle_reg_weight=0.5,
                     loss_center_weight=5.0, loss_size_weight=1.0, loss_no_object_contrast_weight=0.05,
                     loss_predicted_region_embed_l1_weight=1, loss_sem_cls_softmax_skip_none_gt_sample_weight=1,
                     loss_feat_seen_softmax_weakly_loss_with_novel_cate_confi_weight=1,
                     matcher_giou_cost=3, matcher_cls_cost=1, matcher_center_cost=5, matcher_objectness_cost=5,
                     train_range_max=10, confidence_type="clip-max-prob",
                     confidence_type_in_datalayer="clip-max-prob").items():
        setattr(ns, k, v)
    return ns


def synthetic_targets(batch, gen, ngt=64, ncls=10, max_boxes=20):
    """Ground-truth entries of ``batch_data_label`` (datasets/sunrgbd_anonymous_aligned_image.py:455-530) for
    synthetic scenes: 0..max_boxes rotated boxes per scene inside the scene's extent, padded to ngt."""
    from coda_neurips2023_amd.box_util import get_3d_box_batch_tensor
    mn, mx = batch["point_cloud_dims_min"].cpu(), batch["point_cloud_dims_max"].cpu()
    bsz = mn.shape[0]
    nactual = torch.randint(0, max_boxes + 1, (bsz,), generator=gen)
    if bsz > 1:
        nactual[0] = max(int(nactual[0]), 1)  # at least one scene with boxes
    extent = (mx - mn)[:, None]
    centers = mn[:, None] + torch.rand(bsz, ngt, 3, generator=gen) * extent
    sizes = torch.rand(bsz, ngt, 3, generator=gen) * 1.3 + 0.2
    angle_cls = torch.randint(0, 12, (bsz, ngt), generator=gen)
    angle_res = (torch.rand(bsz, ngt, generator=gen) - 0.5) * 0.2
    angles = angle_cls * (2 * np.pi / 12) + angle_res  # class2angle, datasets/...:130-142 (before the wrap)
    cam = torch.stack((centers[..., 0], -centers[..., 2], centers[..., 1]), -1)
    dev = batch["point_clouds"].device
    t = {"gt_box_present": (torch.arange(ngt)[None] < nactual[:, None]).float(),
         "gt_box_sem_cls_label": torch.zeros(bsz, ngt, dtype=torch.int64),
         "gt_box_seen_sem_cls_label": torch.randint(0, ncls, (bsz, ngt), generator=gen),
         "gt_box_seen_sem_cls_confi": torch.ones(bsz, ngt),
         "gt_box_centers_normalized": (centers - mn[:, None]) / extent,
         "gt_box_sizes_normalized": sizes / extent,
         "gt_box_angles": angles.float(), "gt_box_corners": get_3d_box_batch_tensor(sizes, angles.float(), cam),
         "gt_angle_class_label": angle_cls, "gt_angle_residual_label": angle_res}
    return {k: v.to(dev) for k, v in t.items()}


CLIP_GRADIENT = 0.1  # main.py:52 --clip_gradient's default: engine.py:161-162 clips every step


def make_optimizer(params, dry=False, force_torch=False):
    """The tail of the reference's step (engine.py:161-164): clip_grad_norm_(parameters, 0.1), AdamW.step().
    -> (optimizer, clip function).  Default: this package's three-launch kernels (coda_neurips2023_amd.optim);
    CODA_OPTIM=torch: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True) (dev A/B; also the dry run)."""
    params = list(params)
    if dry or force_torch or os.environ.get("CODA_OPTIM", "coda") == "torch":
        opt = torch.optim.AdamW(params, lr=1e-4, fused=not dry)
        return opt, lambda: torch.nn.utils.clip_grad_norm_(params, CLIP_GRADIENT)
    from coda_neurips2023_amd import optim
    opt = optim.AdamW(params, lr=1e-4)
    return opt, lambda: optim.clip_grad_norm_(params, CLIP_GRADIENT)


def synthetic_image_inputs(bsz, dev, seed):
    """What the dataset adds to a batch for the image branch (datasets/sunrgbd_anonymous_aligned_image.py:
    884-899): a 730 x 530 RGB image per scene (random pixels: the tower's cost does not depend on content), a
    SUN RGB-D-like pinhole camera, no augmentation (scale 1, no rotation, no flips)."""
    gen = torch.Generator().manual_seed(seed)
    f64 = dict(dtype=torch.float64)
    eye = torch.eye(3, **f64).expand(bsz, 3, 3).contiguous()
    kmat = torch.tensor([[529.5, 0.0, 365.0], [0.0, 529.5, 265.0], [0.0, 0.0, 1.0]], **f64).expand(bsz, 3, 3).contiguous()
    out = {"input_image": torch.randint(0, 256, (bsz, 530, 730, 3), dtype=torch.uint8, generator=gen),
           "K": kmat, "Rtilt": eye, "rot_array": eye.clone(), "scale_array": torch.ones(bsz, 1, 3, **f64),
           "flip_array": torch.ones(bsz, 1, **f64), "image_flip_array": torch.ones(bsz, 1, **f64),
           "flip_length": torch.full((bsz,), 730.0, **f64), "ori_width": torch.full((bsz,), 730.0, **f64),
           "ori_height": torch.full((bsz,), 530.0, **f64), "y_offset": torch.zeros(bsz, **f64),
           "x_offset": torch.zeros(bsz, **f64)}
    return {k: v.to(dev) for k, v in out.items()}


def build_model_workload(dev, nq=256, config_tag="configs[2]", attn="fp32", image_branch=False, dec_dim=256):
    """configs[2] (and, with nq=512 on 40k-point scenes and bf16 MFMA attention, the one-GPU share of
    configs[4]): the training step as engine.py:144-159 runs it -- model_3detr enc(3L)+dec(8L) forward with
    dropout on (enc/dec 0.1, heads 0.3), ``criterion(outputs, batch_data_label)`` built by ``build_criterion``
    from the stage-2 recipe's flags (gIoU / L1 centre / class / objectness cost matrix for all 8 decoder layers,
    Hungarian assignment, the matched box terms and the two CLIP-space alignment terms, criterion.py:598-644,
    924-943), backward.  Synthetic stand-ins: unit-norm text embeddings for 10 seen classes, unit-norm image-crop
    embeddings / weak labels (the CLIP image branch, SURVEY.md 8f rank 2, is outside the path), random rotated
    ground-truth boxes (0-20 per scene, padded to 64)."""
    import torch.nn.functional as F

    from coda_neurips2023_amd.criterion import build_criterion
    from coda_neurips2023_amd.dataset_config import HotPathDatasetConfig
    from coda_neurips2023_amd.model_3detr import build_model

    torch.manual_seed(0)
    ncls = 10
    gen = torch.Generator().manual_seed(1)
    text = F.normalize(torch.randn(ncls, 512, generator=gen), dim=-1)
    img_emb = F.normalize(torch.randn(B_PER_GPU, nq, 512, generator=gen), dim=-1).to(dev)
    mask = (torch.rand(B_PER_GPU, nq, 1, generator=gen) < 0.25).float().to(dev)  # 32/128 crops per scene
    weak_label = torch.randint(0, ncls, (B_PER_GPU, nq), generator=gen).to(dev)
    weak_conf = (torch.rand(B_PER_GPU, nq, generator=gen) * (torch.rand(B_PER_GPU, nq, generator=gen) < 0.5)).to(dev)

    regions = None
    if image_branch:  # SURVEY.md 8f rank 2 inside the step: project + crop + frozen ViT-B/16 (fp16, random-init weights)
        from coda_neurips2023_amd import clip_crops, clip_tower
        tower = clip_tower.convert_weights(clip_tower.ImageTower(512, 224, 12, 768, 16)).to(dev)
        regions = clip_crops.RegionEmbeddingProvider(tower, distillation_box_num=32, box_pool=128,
                                                     rng=np.random.RandomState(7))

    def provider(inputs, outputs, curr_epoch=-1):
        if regions is not None:
            outputs = regions(inputs, outputs, curr_epoch)
        else:
            outputs["gt_text_correlation_embedding"] = img_emb
            outputs["gt_text_correlation_embedding_mask"] = mask
        outputs["weak_box_cate_label"] = weak_label
        outputs["weak_confidence_weight"] = weak_conf
        return outputs

    cfg = HotPathDatasetConfig()
    args = recipe_args(nq, dec_dim=dec_dim)
    model, _ = build_model(args, cfg, text_features_fg_norm=text, region_embedding_provider=provider)
    model.to(dev).train()
    crit = build_criterion(args, cfg)
    if dev.type == "cpu":  # the CPU port: gIoU from the C oracle, assignment by scipy (the reference's host route)
        from oracle import cpu_port
        crit.giou_fn = cpu_port.generalized_box3d_iou
    crit = crit.to(dev)
    tgt_gen = torch.Generator().manual_seed(2)

    from coda_neurips2023_amd import attention_core

    def step(m, batch, pre_encoded=None, with_dict=False):
        if "gt_box_present" not in batch:  # ground truth travels with the batch (engine.py:137-148); made once
            batch.update(synthetic_targets(batch, tgt_gen))
        # the MFMA operand type of the attention core is a per-call option: a scope around the forward pass, which the
        # backward of the same graph inherits (attention_core.mfma_dtype)
        with attention_core.mfma_dtype(attn) if dev.type == "cuda" else contextlib.nullcontext():
            pred = m(batch, curr_epoch=0, pre_encoded=pre_encoded) if pre_encoded is not None else m(batch, curr_epoch=0)
            loss, loss_dict = crit(pred, batch)
        if _capture is not None:
            _capture.update(loss=loss, loss_dict=loss_dict, outputs=pred["outputs"])
        return (loss, loss_dict) if with_dict else loss

    desc = (f"{config_tag}: full model_3detr (SA {'40000' if nq == 512 else '20000'}->2048 r=0.2 ns=64, enc 3L d=256 "
            f"h=4, dec 8L d={dec_dim} h=4, {nq} queries, 6 heads incl. 512-d CLIP-space head) fwd+bwd, batch=8/GPU, "
            f"{'fp32 tensors, bf16 MFMA attention (fp32 accumulate/softmax)' if attn == 'bf16' else 'fp32'}, dropout on; "
            "loss = criterion(outputs, batch) of the stage-2 recipe for all 8 decoder layers: gIoU + centre + class + "
            "objectness cost matrix, Hungarian assignment (on the device), matched box terms (class CE, angle CE + "
            "Huber, centre / size L1), both CLIP-space alignment terms (10 seen classes, synthetic embeddings); "
            "0-20 synthetic rotated GT boxes per scene")
    return model, step, desc, "model"


def run_image_tower(dev, steps, warmup):
    """SURVEY.md 8f rank 2, measured next to the headline: the frozen CLIP image tower (ViT-B/16, fp16 like the
    reference's) on the crops of one step -- 8 scenes x 32 proposals (models/model_3detr.py:991) -- random-init
    weights (the checkpoint is not in this image), inputs resident in HBM.  Algorithmic flops = the GEMMs and the
    attention products of VisionTransformer.forward; peak = dense fp16 MFMA."""
    from coda_neurips2023_amd import clip_tower
    crops = B_PER_GPU * 32
    torch.manual_seed(0)
    tower = clip_tower.convert_weights(clip_tower.ImageTower(512, 224, 12, 768, 16)).to(dev)
    x = torch.randn(crops, 3, 224, 224, device=dev)
    for _ in range(warmup):
        tower.encode_image(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tower.encode_image(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    l, w, mlp = 197, 768, 3072
    flops = crops * (12 * (2 * l * w * (4 * w + 2 * mlp) + 4 * l * l * w) + 2 * 196 * 768 * w + 2 * w * 512)
    tf = flops / dt / 1e12
    return {"metric": "crops/sec, CLIP ViT-B/16 image tower, fp16 (frozen, forward only)", "value": round(crops / dt, 1),
            "unit": "crops/s", "ms_per_step": round(dt * 1e3, 3), "steps": steps, "warmup": warmup, "dtype": "f16",
            "config": {"workload": "8 scenes x 32 crops of 224x224 (one training step's distillation crops)"},
            "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": 2500.0, "unit": "TFLOP/s",
                         "frac": round(tf / 2500.0, 4), "traffic": None}}


def run_alignment_extra(dev, reps=10):
    """SURVEY.md 8a row a13 at the stage-2 class counts (232 / 1201 prompts, models/model_3detr.py:321): both alignment
    terms of all 8 decoder layers (16 384 proposal rows x 512), forward + backward, on the matrix-core route (class logits
    and their gradient as two dense bf16x3 products, align_loss._AlignLossGemm) and on the one-wave-per-row vector kernel
    the headline's 10 classes use.  Flops = the two dense products, 4 * rows * ncls * 512."""
    from coda_neurips2023_amd import align_loss
    nl, b, nq, e = 8, B_PER_GPU, 256, 512
    rows = nl * b * nq
    gen = torch.Generator().manual_seed(5)
    out = {}
    for ncls in (232, 1201):
        emb = torch.randn(nl, b, nq, e, generator=gen).to(dev).requires_grad_(True)
        gt = torch.nn.functional.normalize(torch.randn(b, nq, e, generator=gen), dim=-1).to(dev)
        wm = (torch.rand(b, nq, generator=gen) < 0.25).float().to(dev)
        text = torch.nn.functional.normalize(torch.randn(ncls, e, generator=gen), dim=-1).to(dev).unsqueeze(0).expand(b, -1, -1)
        labels = torch.randint(0, ncls, (nl, b, nq), generator=gen).to(dev)
        conf = torch.rand(nl, b, nq, generator=gen).to(dev)
        scale = torch.tensor(14.2857, device=dev)
        res = {}
        for route, thr in (("matrix_cores", 64), ("vector_rows", 1 << 30)):
            saved = align_loss.GEMM_MIN_CLASSES
            align_loss.GEMM_MIN_CLASSES = thr

            def one():
                emb.grad = None
                l1, ce = align_loss.align_loss_sums(emb, gt, wm, text, scale, labels, conf)
                (l1.sum() + ce.sum()).backward()

            try:
                for _ in range(2):
                    one()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    one()
                torch.cuda.synchronize()
                res[route] = (time.perf_counter() - t0) / reps
            finally:
                align_loss.GEMM_MIN_CLASSES = saved
        fl = 4.0 * rows * ncls * e
        out[f"ncls_{ncls}"] = {"ms_matrix_cores": round(res["matrix_cores"] * 1e3, 4),
                               "ms_vector_rows": round(res["vector_rows"] * 1e3, 4),
                               "tflops_matrix_cores": round(fl / res["matrix_cores"] / 1e12, 1),
                               "speedup": round(res["vector_rows"] / res["matrix_cores"], 2)}
    out["what"] = ("both CLIP-space alignment terms of 8 layers x 8 scenes x 256 proposals, forward + backward (wall time per "
                   "call incl. the row-wise kernels and the per-call split of the prompt matrix)")
    return out


def run_extra(kind, dev, steps, warmup):
    """The other single-GPU configurations of BASELINE.json next to the headline, so that the driver's default
    command times them too: configs[1] (set abstraction only) and the one-GPU share of configs[4] (40 000-point
    scenes, 512 queries, bf16 MFMA attention).  Same loop as the headline: `warmup` untimed steps, `steps` timed
    steps between synchronisations, optimizer step inside, inputs resident in HBM."""
    from coda_neurips2023_amd import attention_core
    n_points = N_POINTS
    prefetch = False
    sa_prefetcher = None
    if kind in ("sa", "sa_prefetch"):
        mod, step_fn, desc, _ = build_workload("sa", dev)
        if kind == "sa_prefetch":
            # the module's own split: prepare(xyz) = the parameter-free front (FPS, centre gather, ball query + grouping,
            # packing) of batch i + 1 on the sampling side stream during step i, forward(xyz, prepared=...) continues
            # from it -- what the full model's prefetch_sampling does for its pre-encoder
            from coda_neurips2023_amd.pointnet2.pointnet2_utils import SamplingPrefetcher
            sa_prefetcher = SamplingPrefetcher()

            def step_fn(model, batch, _inner=None):  # noqa: F811
                pc = batch["point_clouds"]
                front = sa_prefetcher.take(pc)
                _, feat, _ = model(pc if front is None else front["xyz"], prepared=front)
                return feat.square().mean()
    elif kind == "scripts":
        mod, step_fn, desc, _ = build_model_workload(dev, nq=128, dec_dim=512,
                                                     config_tag="the scripts' variant (scripts/coda_sunrgbd_stage1.sh: "
                                                                "dec_dim 512, 128 queries; SURVEY.md 8d)")
        prefetch = True
    elif kind == "distill":
        mod, step_fn, desc, _ = build_model_workload(dev, config_tag="configs[2] + the CLIP image branch", image_branch=True)
        desc += ("; image branch inside the step: box projection, 8 x 32 crops, frozen ViT-B/16 image tower (fp16, "
                 "random-init), models/model_3detr.py:902-1086")
        prefetch = True
    else:
        n_points = 40000
        mod, step_fn, desc, _ = build_model_workload(dev, nq=512, config_tag="configs[4], one GPU's share", attn="bf16")
        prefetch = True
    pool = []
    for i in range(3):
        pc, mn, mx = make_batch(B_PER_GPU, n_points, seed=4321 + i)
        pool.append({"point_clouds": torch.from_numpy(pc).to(dev), "point_cloud_dims_min": torch.from_numpy(mn).to(dev),
                     "point_cloud_dims_max": torch.from_numpy(mx).to(dev)})
        if kind == "distill":
            pool[-1].update(synthetic_image_inputs(B_PER_GPU, dev, seed=99 + i))
    opt, clip = make_optimizer(mod.parameters())

    def one(i):
        if prefetch:
            mod.prefetch_sampling(pool[(i + 1) % len(pool)], wait_for=None)
        if sa_prefetcher is not None:
            sa_prefetcher.submit(pool[(i + 1) % len(pool)]["point_clouds"], mod, wait_for=None)
        opt.zero_grad(set_to_none=True)
        step_fn(mod, pool[i % len(pool)]).backward()
        clip()
        opt.step()

    for i in range(warmup):
        one(i)
    attn_ms = {}
    if kind == "model40k":
        attention_core.enable_kernel_timing(0)
    # as in the headline loop: a full pass of Python's cyclic collector over the long-lived objects of torch + the
    # models built so far costs 40-90 ms -- inside ten timed steps that is +4..9 ms per step (seen once in round 5:
    # 24.5 instead of 16.9 ms per step on this configuration with identical kernel times)
    gc.collect()
    gc.freeze()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if kind == "model40k":
        attn_ms = attention_core.collect_kernel_timing()
        attention_core.disable_kernel_timing()
    out = {"metric": "scenes/sec fwd+bwd", "value": round(B_PER_GPU * steps / dt, 3), "unit": "scenes/s", "n_gpus": 1,
           "steps": steps, "warmup": warmup, "ms_per_step": round(dt / steps * 1e3, 4),
           "config": {"workload": desc, "scenes_per_gpu": B_PER_GPU, "points": n_points,
                      "sampling": "FPS + ball query of batch i+1 on a side stream during step i"
                                  if (prefetch or sa_prefetcher is not None) else "in line"}}
    if attn_ms:
        # bf16 MFMA: executed flops over the dense bf16 peak; these kernels are bound by the softmax VALU work and
        # by K/V delivery, not by the matrix cores
        kern = {}
        for (k, l, s_len), samples in sorted(attn_ms.items(), key=lambda kv: (-kv[0][1] * kv[0][2], kv[0][0])):
            if k in ("delta", "dqr", "ktp"):
                continue
            ms = sum(samples) / len(samples)
            tf = ATTN_FLOPS[k] * l * s_len * 256 * B_PER_GPU / (ms * 1e-3) / 1e12
            kern[f"{k}_{l}x{s_len}"] = {"avg_launch_ms": round(ms, 5), "achieved_tflops": round(tf, 1),
                                        "frac_of_bf16_mfma_peak": round(tf / MFMA_BF16_PEAK_TFLOPS, 4)}
        out["attention_kernels_bf16"] = kern
    del mod, opt, pool
    torch.cuda.empty_cache()
    return out


def cpu_baseline(kind):
    """The same step on the host cores: the product's host-side module graph with the CPU
    oracle (oracle/pointnet2_oracle.c ops, plain torch attention) patched into its kernel
    seams (oracle/cpu_port.py), torch CPU threads = all cores, bounded sample (1 scene)."""
    from oracle import cpu_port
    from oracle import pointnet2_oracle as O
    O.build()
    # torch-CPU ops of this size stop scaling (and start thrashing) beyond a few dozen threads:
    # use at most 32 and report exactly that count
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    global B_PER_GPU
    saved_b = B_PER_GPU
    B_PER_GPU = 1  # bounded sample: one scene per step
    try:
        cpu = torch.device("cpu")
        mod, step_fn, _, _ = build_workload(kind, cpu)
        pc, mn, mx = make_batch(1, N_POINTS, seed=4242)
        batch = {"point_clouds": torch.from_numpy(pc), "point_cloud_dims_min": torch.from_numpy(mn),
                 "point_cloud_dims_max": torch.from_numpy(mx)}

        def one():
            mod.zero_grad(set_to_none=True)
            step_fn(mod, batch).backward()

        # (`batch` is rebound below: closure reads the current binding)

        with cpu_port.patched():
            # lazy-init warm-up on a 10x smaller cloud, then timed full-size reps within ~20 s
            small, smn, smx = make_batch(1, N_POINTS // 10, seed=7)
            full, batch = batch, {"point_clouds": torch.from_numpy(small),
                                  "point_cloud_dims_min": torch.from_numpy(smn),
                                  "point_cloud_dims_max": torch.from_numpy(smx)}
            one()
            batch = full
            t0 = time.perf_counter()
            reps = 0
            while reps < 1 or (time.perf_counter() - t0 < 20.0 and reps < 20):
                one()
                reps += 1
            dt = (time.perf_counter() - t0) / reps
    finally:
        B_PER_GPU = saved_b
    return {"value": round(1.0 / dt, 4), "unit": "scenes/s", "cores": cores, "kind": "port",
            "sample": f"{reps} x 1 scene (20000 pts) fwd+bwd of the same workload: oracle C ops (scalar, "
                      f"OpenMP over scenes) + torch-CPU layers on {cores} threads"}


def _arithmetic_note():
    from coda_neurips2023_amd import fused_layers, gemm
    dense = ("dense projections with >= 8192 token rows (y = x W^T + b, dx = dy W): fp32 operands as three bf16 pieces, "
             "six piece products on the bf16 matrix cores, fp32 accumulate (csrc/gemm_x3.hip)" if gemm._X3 else
             "dense projections: library fp32 GEMMs")
    wgrad = "weight gradients: bf16x3 kernel" if (gemm._X3 and gemm._X3_TN) else "weight gradients: library fp32 GEMMs"
    attn = ("encoder self-attention forward: bf16x3 mode of the fused core; every attention backward and the decoder's "
            "cores: fp32 MFMA" if fused_layers._FWD_X3 else "attention cores: fp32 MFMA")
    return "; ".join((dense, wgrad, attn))


def compact_line(out, dry=False):
    """The whole record goes to a file (CODA_BENCH_FULL, default gpurun_out/bench_full.json when that directory exists,
    else bench_full.json beside this script); stdout gets ONE line that stays under the 8 KB tail the driver keeps:
    everything the contract names, `roofline` (with the north-star scalars), `cpu_baseline`, and of the secondary
    blocks one number each."""
    full = json.dumps(out)
    if not dry:
        path = os.environ.get("CODA_BENCH_FULL")
        if not path:
            d = os.path.join(ROOT, "gpurun_out")
            path = os.path.join(d if os.path.isdir(d) else ROOT, "bench_full.json")
        try:
            with open(path, "w") as f:
                f.write(full + "\n")
        except OSError as e:  # a read-only tree must not cost the line
            print(f"bench.py: full record not written ({e})", file=sys.stderr)
            path = None
        short = dict(out)
        short.pop("value_unchanged_caller", None)
        others = short.pop("roofline_others", None)
        if others:
            short["roofline_others"] = {"count": len(others), "where": "full record"}
        extras = short.pop("extra_configs", None)
        if extras:
            brief = {}
            for name, e in extras.items():
                brief[name] = {"value": e.get("value"), "unit": e.get("unit"), "ms_per_step": e.get("ms_per_step"),
                               "steps": e.get("steps")}
                for k, v in (e.get("attention_kernels_bf16") or {}).items():
                    brief[name].setdefault("attention_bf16_us", {})[k] = round(v["avg_launch_ms"] * 1e3, 1)
                if isinstance(e.get("roofline"), dict):
                    brief[name]["frac"] = e["roofline"].get("frac")
                if name == "alignment_loss_stage2_classes":
                    brief[name] = {k: v for k, v in e.items() if k != "what"}
            short["extra_configs"] = brief
        short["full_record"] = os.path.relpath(path, ROOT) if path else None
        return json.dumps(short)
    return full


class DeferredFiniteCheck:
    """engine.py:155-157 stops the training on a non-finite loss with ``loss_reduced.item()``: a device-to-host
    read-back that parks the host until the whole forward pass has executed, every step.  The headline loop keeps the
    check but defers it by one step: the loss goes to pinned host memory asynchronously and the PREVIOUS step's value
    (long complete) is examined -- the run still stops, one step later, and the host never waits.  (The unchanged
    caller's leg below keeps the reference's blocking form.)"""

    def __init__(self, dev):
        self.host = [torch.zeros(1, dtype=torch.float32).pin_memory() for _ in range(2)]
        self.events = [None, None]
        self.turn = 0

    def push(self, loss):
        prev = self.turn ^ 1
        if self.events[prev] is not None:
            self.events[prev].synchronize()  # recorded a whole step ago
            if not math.isfinite(float(self.host[prev][0])):
                print("Loss in not finite. Training will be stopped.", file=sys.stderr)
                sys.exit(1)
        self.host[self.turn].copy_(loss.detach().reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[self.turn] = ev
        self.turn = prev


def reference_loss_sync(loss, loss_dict):
    """engine.py:152-157, verbatim in effect: the loss averaged over the ranks, the loss dictionary reduced, and the
    blocking finite check on the host."""
    from coda_neurips2023_amd.dist_utils import all_reduce_average, reduce_dict
    loss_reduced = all_reduce_average(loss)
    loss_dict_reduced = reduce_dict(loss_dict)
    if not math.isfinite(loss_reduced.item()):
        print("Loss in not finite. Training will be stopped.", file=sys.stderr)
        sys.exit(1)
    return loss_reduced, loss_dict_reduced


def make_batch_t(bsz, n, seed, dev):
    pc, _, _ = make_batch(bsz, n, seed=seed)
    return torch.from_numpy(pc).to(dev)[..., :3].contiguous()


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs: all files together
DUMP_SAMPLE = 1 << 22  # elements kept of the flattened parameters / gradients (a fixed, seeded sample)


def training_state(model, opt, dev):
    """--dump-outputs: copies of all that a step reads and changes -- parameters and buffers, the optimizer's state,
    the generators dropout draws its seeds from -- taken after the warm-up and put back before the timed region, so
    that the timed steps start from the same state whatever number of settle steps ran in between."""
    return {"model": {k: v.detach().clone() for k, v in model.state_dict().items()},
            "opt": {p: {k: v.clone() if torch.is_tensor(v) else v for k, v in st.items()} for p, st in opt.state.items()},
            "cpu_rng": torch.get_rng_state(),
            "cuda_rng": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None}


def restore_training_state(model, opt, state, dev):
    model.load_state_dict(state["model"])  # copies into the existing parameters: the optimizer keeps its references
    for p in [p for p in opt.state if p not in state["opt"]]:
        del opt.state[p]
    for p, st in state["opt"].items():
        cur = opt.state[p]
        for k, v in st.items():
            if torch.is_tensor(v) and torch.is_tensor(cur.get(k)) and cur[k].shape == v.shape:
                cur[k].copy_(v)
            else:
                cur[k] = v.clone() if torch.is_tensor(v) else v
    torch.set_rng_state(state["cpu_rng"])
    if state["cuda_rng"] is not None:
        torch.cuda.set_rng_state(state["cuda_rng"], dev)


def _dump_array(t):
    t = t.detach()
    t = t.double() if not t.is_floating_point() or t.dtype == torch.float64 else t.float()
    return t.cpu().numpy()


def _fixed_sample(flat):
    n = flat.numel()
    if n <= DUMP_SAMPLE:
        return flat
    idx = np.sort(np.random.default_rng(0).permutation(n)[:DUMP_SAMPLE])
    return flat[torch.from_numpy(idx).to(flat.device)]


def dump_outputs(path, captured, model):
    """--dump-outputs: what the last timed step computed, as a caller of the step receives it -- the loss, the loss
    terms, the predictions of the last decoder layer (the set-abstraction features for --workload sa) and the updated
    model: the parameters after the optimizer step and the (clipped) gradients it applied, both flattened in
    ``named_parameters`` order and sampled at fixed positions.  float32 (float64 for integer results), one
    DIR/<name>.npy per array."""
    arrays = {"loss": captured["loss"]}
    for k, v in (captured.get("loss_dict") or {}).items():
        if torch.is_tensor(v):
            arrays[k if k.startswith("loss") else "loss_" + k] = v
    for k, v in (captured.get("outputs") or {}).items():
        if torch.is_tensor(v):
            arrays["out_" + k] = v
    params = [p for p in model.parameters() if p.requires_grad]
    arrays["param_sample"] = _fixed_sample(torch.cat([p.detach().reshape(-1) for p in params]))
    arrays["grad_sample"] = _fixed_sample(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p))
                                                     .detach().reshape(-1) for p in params]))
    arrays = {re.sub(r"[^A-Za-z0-9_.-]", "_", k): _dump_array(v) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        sys.exit(f"bench.py: --dump-outputs would write {total} bytes, more than {DUMP_MAX_BYTES}")
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)
    return {"dir": path, "files": len(arrays), "bytes": total}


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def spawn_ranks(n):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks here, one process per GPU, the way
    the reference starts its own (main.py:1103-1108, torch.multiprocessing.spawn(main, nprocs=ngpus)) -- every child
    is this same command line with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in its environment, i.e. exactly what
    `python -m torch.distributed.run --nproc-per-node N bench.py ...` would have started.  Rank 0's JSON line goes to
    the inherited stdout.  The first rank that fails takes the others down and its exit code becomes ours."""
    import subprocess
    env = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=os.environ.get("MASTER_PORT") or str(_free_port()), CODA_BENCH_SPAWNED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL's intra-node transport needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(n)]
    rc = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} of {n} exited with {code}; stopping the other ranks", file=sys.stderr)
                for q in live:
                    procs[q].terminate()
        time.sleep(0.05)
    return rc


def main():
    global _capture
    args = parse()
    dry = os.environ.get("CODA_BENCH_DRY") == "1"  # control-flow test on CPU, see build_dry_workload()
    if args.gpus < 1:
        sys.exit(f"bench.py: --gpus {args.gpus}")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if not dry and os.environ.get("CODA_BENCH_ONE_DEVICE") != "1" and torch.cuda.device_count() < args.gpus:
            sys.exit(f"bench.py: --gpus {args.gpus} but this node shows {torch.cuda.device_count()} GPU(s)")
        sys.exit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # a rank count that differs from --gpus must never produce a line (a one-rank run labelled as N GPUs or the reverse)
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to measure")
    assert dry or torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback exists)"
    # dev-only smoke mode for 1-GPU boxes: all ranks on cuda:0 over gloo (RCCL refuses two ranks per
    # device); exercises the DDP + SyncBatchNorm code path, its numbers mean nothing
    one_device = os.environ.get("CODA_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    elif not dry and torch.cuda.device_count() < world:
        sys.exit(f"bench.py: {world} ranks but this node shows {torch.cuda.device_count()} GPU(s): one process per GPU")
    if dry:
        dev = torch.device("cpu")
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)

    def sync():
        if not dry:
            torch.cuda.synchronize()

    # CODA_BENCH_FORCE_DDP=1 (development check on a single GPU): a one-rank RCCL group, so that the SyncBatchNorm +
    # DistributedDataParallel wrapping of the multi-GPU runs is exercised by the same command
    force_ddp = world == 1 and os.environ.get("CODA_BENCH_FORCE_DDP") == "1" and not dry
    if force_ddp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_device or dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    if world > 1 and dist.get_world_size() != args.gpus:
        sys.exit(f"bench.py: process group of {dist.get_world_size()} ranks for --gpus {args.gpus}")

    if os.environ.get("CODA_BLAS"):  # dev A/B: "cublas" (= rocBLAS) | "cublaslt" (= hipBLASLt, torch's default here)
        torch.backends.cuda.preferred_blas_library(os.environ["CODA_BLAS"])
    mod, step_fn, desc, kind = build_workload(args.workload, dev)
    if dry and os.environ.get("CODA_BENCH_DRY_FAIL_RANK") == str(rank):  # tests/test_bench_dry.py: a rank that dies
        sys.exit(f"bench.py: rank {rank} fails on request")
    model = mod
    reducer = None
    if world > 1 or force_ddp:
        # reference: SyncBatchNorm + DDP (main.py:993-996)
        model = mod if dry else torch.nn.SyncBatchNorm.convert_sync_batchnorm(mod)  # (SyncBN needs GPU modules)
        ddp_mode = "default" if dry else os.environ.get("CODA_DDP", "flat")
        if ddp_mode == "flat":
            # this package's gradient synchronisation: one pack launch + ONE all-reduce of the flat 31.6 MB buffer
            # after backward, p.grad = views of it (optim.FlatGradReducer); forced onto one rank (RCCL all-reduce
            # executed): 444 scenes/s against 425 under DistributedDataParallel with bucket views (CODA_DDP=tuned) and
            # torch's defaults (CODA_DDP=default)
            from coda_neurips2023_amd.optim import FlatGradReducer
            # two segments: heads + decoder (81 % of the bytes) are packed and all-reduced from a backward hook as
            # soon as the decoder node's gradients have landed, i.e. under the projection / encoder / set-abstraction
            # backward; the rest after backward.  CODA_DDP_OVERLAP=0: both after backward (A/B)
            reducer = FlatGradReducer(model, broadcast=False, early=("mlp_heads.", "decoder."),
                                      overlap=os.environ.get("CODA_DDP_OVERLAP", "1") != "0")
            if world > 1:
                reducer.sync_parameters(model)  # rank 0's parameters AND buffers, like DDP's constructor
        else:
            ddp_kw = {}
            if ddp_mode != "default":
                # gradients live in the all-reduce buckets, two buckets of ~16 MB so that the first all-reduce overlaps
                # the encoder's backward
                ddp_kw = dict(gradient_as_bucket_view=True, bucket_cap_mb=int(os.environ.get("CODA_DDP_BUCKET_MB", "16")),
                              static_graph=os.environ.get("CODA_DDP_STATIC", "0") == "1")
            model = torch.nn.parallel.DistributedDataParallel(model, device_ids=None if dry else [local_rank], **ddp_kw)

    # synthetic inputs, resident in HBM before timing; a few distinct batches cycle
    pool = []
    for i in range(4):
        n_points = 64 if dry else (40000 if args.workload == "model40k" else N_POINTS)
        pc, mn, mx = make_batch(B_PER_GPU, n_points, seed=1234 + rank * 1000 + i)
        pool.append({"point_clouds": torch.from_numpy(pc).to(dev),
                     "point_cloud_dims_min": torch.from_numpy(mn).to(dev),
                     "point_cloud_dims_max": torch.from_numpy(mx).to(dev)})
    raw_model = model.module if hasattr(model, "module") else model
    opt, clip_gradients = make_optimizer(model.parameters(), dry)
    prefetch = args.prefetch == "on" and kind == "model"

    finite = DeferredFiniteCheck(dev) if not dry else None

    # extra host time per step: CODA_BENCH_HOST_SPIN_US (dev probe) and the slack probe behind the settle blocks below
    spin = {"s": float(os.environ.get("CODA_BENCH_HOST_SPIN_US", "0")) * 1e-6}

    def one_step_eager(i):
        if spin["s"]:
            t_end = time.perf_counter() + spin["s"]
            while time.perf_counter() < t_end:
                pass
        if prefetch:
            # the data pipeline knows the next batch: its furthest point sampling (8 workgroups,
            # ~3.4 ms of dependent rounds) runs on a side stream while this step computes
            raw_model.prefetch_sampling(pool[(i + 1) % len(pool)], wait_for=None)  # batches are resident
        opt.zero_grad(set_to_none=True)
        loss = step_fn(model, pool[i % len(pool)])
        if finite is not None or world > 1:
            # engine.py:152-157: the exit decision is taken on the loss AVERAGED OVER THE RANKS, so that every rank takes
            # the same one (a rank leaving alone would park the others in their next collective); one scalar
            # all-reduce, enqueued like any kernel.  Then the check itself, one step late and without a host stall
            seen = loss.detach()
            if world > 1:
                seen = seen.clone()
                dist.all_reduce(seen)
                seen /= world
            if finite is not None:
                finite.push(seen)
        loss.backward()
        if reducer is not None:
            reducer.reduce()
        clip_gradients()
        opt.step()

    graph = None  # (a hipGraph replay of the step is not available on this stack: DESIGN.md section 7)
    one_step = one_step_eager

    for i in range(args.warmup):
        one_step(i)
    state_after_warmup = training_state(raw_model, opt, dev) if args.dump_outputs else None

    # Settle: a fresh box can run the first seconds of a process with a host side ~1.4x slower than its steady state
    # (lazy loading of the libraries' code objects, page-ins: seen on 1 of 14 boxes in round 6 -- 413 instead of 557
    # scenes/s in the first timed region of the process, every later leg of the same process at its normal rate, kernel
    # times identical).  After the W warm-up steps, untimed blocks of 5 steps run until a block is within 3 % of the best
    # block so far (at least two blocks, at most 80 = ~6 s); the count goes into the line (host.settle_steps).  The timed
    # region below is unchanged: exactly K steps between barriers + synchronize.
    # Round 6, last part: steadiness of consecutive blocks is not enough.  The FIRST seconds of a process run the whole step
    # 2-25 % slower at a perfectly steady rate (kernel times normal or better -- the GPU idles between them --, the slack
    # probe below reads GPU-bound; the same box's later processes, and this process half a minute later, run at the full
    # rate: 579 / 602 / 618 right after the GPU suite against 625-629 in every later process of those boxes,
    # tools/headline_spread.sh; 470-480 in the very first process of several fresh boxes).  The blocks therefore also run
    # for at least CODA_BENCH_SETTLE_S seconds (default 6; ~450 untimed steps), at most 240 blocks; host.settle_s reports it.
    settle_steps = 0
    settle_s = 0.0
    if not dry and kind == "model" and os.environ.get("CODA_BENCH_SETTLE", "1") != "0":
        best = None
        min_s = float(os.environ.get("CODA_BENCH_SETTLE_S", "6"))
        t_settle = time.perf_counter()
        for _blk in range(240):  # (with several ranks every rank must run the same number of blocks: decisions on reduced values)
            sync()
            t_blk = time.perf_counter()
            for i in range(5):
                one_step(args.warmup + settle_steps + i)
            sync()
            blk = (time.perf_counter() - t_blk) / 5
            settle_steps += 5
            settle_s = time.perf_counter() - t_settle
            if world > 1:  # every rank must take the same decision
                t = torch.tensor([blk, settle_s], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                blk, settle_s = float(t[0].item()), float(t[1].item())
            if best is not None and blk <= best * 1.03 and settle_steps >= 10 and settle_s >= min_s:
                break
            best = blk if best is None else min(best, blk)

    # Host slack.  The step needs ~11 ms of host time for ~13 ms of GPU time: it is GPU-bound with < 2 ms to spare, and a
    # box that is still busy with its own start-up (image page-ins, another tenant's job on the host's cores) runs the
    # first process host-bound -- 482 scenes/s with 16.2 ms of enqueue time per step measured on one box whose later
    # processes read 602.  Probe: five steps as they are against five steps with 1.5 ms of busy-waiting added to the host
    # side of each; a GPU-bound step hides the addition (difference ~0.1 ms), a host-bound one shows it in full.  While
    # it shows (> 1.0 ms) the bench sleeps 5 s and probes again, at most 12 times (2 in a plain run, which stays within
    # half a minute outside its steps); both figures go into the line (host.slack_probe_ms, host.wait_s).  Untimed,
    # like the settle blocks; the timed region is unchanged.
    slack_probe_ms, host_wait_s = None, 0.0
    if not dry and kind == "model" and os.environ.get("CODA_BENCH_HOST_WAIT", "1") != "0":
        base_spin = spin["s"]

        def probe_block(extra):
            nonlocal settle_steps
            spin["s"] = base_spin + extra
            sync()
            t_blk = time.perf_counter()
            for i in range(5):
                one_step(args.warmup + settle_steps + i)
            sync()
            spin["s"] = base_spin
            settle_steps += 5
            return (time.perf_counter() - t_blk) / 5

        attempts = 13 if args.full else 3
        for attempt in range(attempts):
            diff = probe_block(1.5e-3) - probe_block(0.0)
            if world > 1:  # every rank must take the same decision
                t = torch.tensor([diff], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                diff = float(t.item())
            slack_probe_ms = diff * 1e3
            if diff < 1.0e-3 or attempt == attempts - 1:
                break
            time.sleep(5.0)
            host_wait_s += 5.0

    if state_after_warmup is not None:
        sync()
        restore_training_state(raw_model, opt, state_after_warmup, dev)
        del state_after_warmup

    # the set-abstraction stage (and its side-stream sampling) is enqueued eagerly in both modes
    timing = _ext.enable_kernel_timing(["query_and_group_xyz", "ball_query", "furthest_point_sampling"])
    # every rank records (same overhead on all ranks); rank 0 reports
    attn_timed = kind in ("model", "dry")
    if attn_timed:
        from coda_neurips2023_amd import attention_core
    if attn_timed and graph is None:
        # the DOMINANT kernel only (the encoder's dK/dV kernel: 3 launches per step) inside the timed region.  A
        # dispatch that carries events leaves 5-9 us of idle queue on either side of it in the kernel trace (its own
        # completion signal); with all 12 long-sequence launches of a step timed the measurement itself cost the
        # headline 1.5 % (CODA_BENCH_TIMED_KINDS=all: that form, none: no events at all -- same-box A/B).  The other
        # attention kernels are timed in the extra steps behind the timed region, like the decoder's
        sel = os.environ.get("CODA_BENCH_TIMED_KINDS", "dkv")
        if sel == "all":
            attention_core.enable_kernel_timing(1024)
        elif sel != "none":
            attention_core.enable_kernel_timing(1024, kinds=sel.split(","))
    # Python's cyclic collector: a full pass over the ~2e5 long-lived objects of torch + the model costs
    # 40-90 ms of host time, which would land in one unlucky step.  Collect now and move everything that
    # survived the warm-up to the permanent generation (young-generation passes stay on); what the collector
    # still costs inside the timed region is measured and reported.
    gc.collect()
    gc.freeze()
    gc_stat = {"n": 0, "ms": 0.0, "t": 0.0}

    def gc_probe(phase, info):
        if phase == "start":
            gc_stat["t"] = time.perf_counter()
        else:
            gc_stat["n"] += 1
            gc_stat["ms"] += (time.perf_counter() - gc_stat["t"]) * 1e3

    gc.callbacks.append(gc_probe)
    if world > 1:
        dist.barrier()
    if args.dump_outputs:
        _capture = {}  # every timed step refills it: the last one's results remain
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        one_step(i)
    t_host = time.perf_counter() - t0  # the host thread is done enqueueing; the GPU may still be working
    sync()
    if world > 1:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    gc.callbacks.remove(gc_probe)
    _ext.disable_kernel_timing()
    captured, _capture = _capture, None
    dumped = dump_outputs(args.dump_outputs, captured, raw_model) if captured is not None and rank == 0 else None
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    attn_ms, attn_ms_all = {}, {}
    sa_ms, sa_rows = {}, []
    if attn_timed and graph is None:
        attn_ms = attention_core.collect_kernel_timing()
        attention_core.disable_kernel_timing()
    # Extra steps for the other attention kernels: single-process runs only.  A step contains the DDP
    # gradient all-reduce and the SyncBatchNorm exchange, so with several ranks every rank would have to run
    # them in lockstep; the multi-GPU lines report the dominant kernel (timed above) and the ball query only.
    if attn_timed and world == 1 and args.full:
        # every attention kernel (decoder shapes too), `steps` more EAGER steps outside the timed region.  When
        # the timed region replayed a hipGraph these also stand in for the dominant kernel: HIP events cannot
        # be read back from inside a graph replay (the rocprofv3 trace of the same command under profiles/
        # does see the replayed kernels and is the cross-check)
        attention_core.enable_kernel_timing(0)
        from coda_neurips2023_amd.pointnet2 import fused_sa_mlp
        sa_events = fused_sa_mlp.enable_kernel_timing()  # the MFMA GEMM kernels of the set-abstraction MLP
        for i in range(args.steps):
            one_step_eager(i)
        sync()
        attn_ms_all = attention_core.collect_kernel_timing()
        attention_core.disable_kernel_timing()
        fused_sa_mlp.disable_kernel_timing()
        sa_rows = [int(t.item()) for t in sa_events.pop("rows", [])]
        sa_ms = {k: sum(a.elapsed_time(b) for a, b in v) / len(v) for k, v in sa_events.items() if v}
        if graph is not None:
            attn_ms = attn_ms_all

    def avg_ms(name, store=None):
        ev = (timing if store is None else store).get(name, [])
        return sum(s.elapsed_time(e) for s, e in ev) / len(ev) if ev else None

    # The same step as an UNCHANGED engine.py runs it (engine.py:136-164, main.py:993-996): no `prefetch_sampling` call,
    # the loss averaged over the ranks + reduce_dict + the BLOCKING `.item()` finite check of engine.py:152-157 between
    # forward and backward, torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW instead of this package's three-launch
    # tail, and with several ranks the reference's own wrap: SyncBatchNorm.convert_sync_batchnorm +
    # DistributedDataParallel(model, device_ids=[local_rank], find_unused_parameters=False).  Every rank runs it in
    # lockstep, `steps` steps right after the headline's, same barrier + synchronize bracket, max over ranks.
    unchanged = None
    # CODA_BENCH_LEGS=headline: dev switch for kernel traces of the headline leg alone (tools/trace_gaps.py)
    if args.full and kind in ("model", "dry") and os.environ.get("CODA_BENCH_LEGS", "both") != "headline":
        model_u = model
        if reducer is not None:
            reducer.remove_hooks()
            model.zero_grad(set_to_none=True)  # the gradients were views of the reducer's flat buffer
        if world > 1 and not isinstance(model, torch.nn.parallel.DistributedDataParallel):
            model_u = torch.nn.parallel.DistributedDataParallel(model, device_ids=None if dry else [local_rank],
                                                                find_unused_parameters=False)
        opt2, clip2 = make_optimizer(model_u.parameters(), dry=dry, force_torch=True)

        def plain_step(i):
            opt2.zero_grad()
            loss, loss_dict = step_fn(model_u, pool[i % len(pool)], with_dict=True)
            reference_loss_sync(loss, loss_dict)
            loss.backward()
            clip2()
            opt2.step()

        def time_unchanged():
            for i in range(3):
                plain_step(i)
            if world > 1:
                dist.barrier()
            sync()
            t1 = time.perf_counter()
            for i in range(args.steps):
                plain_step(i)
            sync()
            if world > 1:
                dist.barrier()
            sync()
            dt = time.perf_counter() - t1
            if world > 1:
                t = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            return dt

        dt2 = time_unchanged()
        unchanged_at_s = time.perf_counter() - T_PROCESS_START
        unchanged = {"value": round(world * B_PER_GPU * args.steps / dt2, 3), "unit": "scenes/s",
                     "ms_per_step": round(dt2 / args.steps * 1e3, 4),
                     "what": "the same step through the reference's unchanged call sequence (engine.py:136-164): "
                             "model(batch) / criterion / all_reduce_average(loss) + reduce_dict(loss_dict) + the "
                             "blocking loss.item() finite check / backward / torch clip_grad_norm_ + torch AdamW, no "
                             "sampling prefetch" + (", SyncBatchNorm + torch DistributedDataParallel (main.py:993-996)"
                                                    if world > 1 else "")}

    # Multi-GPU diagnostics (rank 0 reports, every rank takes part): the collectives of a step timed in isolation with
    # HIP events -- the two segments of the flat gradient all-reduce and one SyncBatchNorm statistics all-reduce --
    # so that the first scaling run shows where a shortfall comes from.
    # always present, so that a line measured on fewer ranks than asked for cannot pass for an N-GPU line
    comm = {"backend": None, "rccl_ranks": 1, "launched_by": "single process"}
    if world > 1 or force_ddp:
        def timed_allreduce(t, reps):
            if not dry:
                torch.cuda.synchronize()
            if dist.get_world_size() > 1:
                dist.barrier()
            t0 = time.perf_counter()
            for _ in range(reps):
                dist.all_reduce(t)
            if not dry:
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3

        comm = {"backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(),
                "launched_by": ("bench.py itself (one child process per GPU, main.py:1103-1108's form)"
                                if os.environ.get("CODA_BENCH_SPAWNED") == "1" else "an external launcher (torchrun)"),
                "headline_collectives_per_step": "SyncBatchNorm statistics + the flat gradient all-reduce + one scalar "
                                                 "all-reduce of the loss (engine.py:152) for the deferred finite check; "
                                                 "reduce_dict(loss_dict) (engine.py:153, logging only) is NOT in the "
                                                 "headline leg -- it is in value_unchanged"}
        if args.full:  # the collectives timed alone
            reps = 10
            if reducer is not None:
                names = ["early", "late"] if len(reducer.segments) == 2 else [str(k) for k in range(len(reducer.segments))]
                comm["allreduce_ms"] = {n: round(timed_allreduce(seg.flat, reps), 4) for n, seg in zip(names, reducer.segments)}
                comm["allreduce_bytes"] = {n: seg.flat.numel() * 4 for n, seg in zip(names, reducer.segments)}
            else:
                flat = torch.zeros(sum(p.numel() for p in raw_model.parameters() if p.requires_grad), device=dev)
                comm["allreduce_ms"] = {"all": round(timed_allreduce(flat, reps), 4)}
                comm["allreduce_bytes"] = {"all": flat.numel() * 4}
            small = torch.zeros(512, dtype=torch.float64, device=dev)  # [sum, sum of squares] of a 256-channel layer
            one = timed_allreduce(small, 50)
            comm["syncbn_allreduce_ms_each"] = round(one, 4)
            comm["syncbn_collectives_per_step"] = 16  # 8 BatchNorm layers x (forward statistics + backward sums)
            comm["syncbn_ms"] = round(16 * one, 4)

    alone = {}
    if rank == 0 and prefetch and args.full:
        # with the sampling prefetch the operator ran on a side stream, competing with the step's own
        # kernels for CUs: also time it with the GPU to itself, `steps` launches on the same inputs
        alone = _ext.enable_kernel_timing(["query_and_group_xyz"])
        with torch.no_grad():
            for i in range(args.steps):
                xyz = pool[i % len(pool)]["point_clouds"][..., :3].contiguous()
                inds = _ext.furthest_point_sampling(xyz, M_CENTRES)
                new_xyz = torch.gather(xyz, 1, inds.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
                torch.cuda.synchronize()
                _ext.query_and_group_xyz(new_xyz, xyz, RADIUS, NSAMPLE, True, channels_last=True)
        torch.cuda.synchronize()
        _ext.disable_kernel_timing()

    # the same operator with the GLOBAL batch on one GPU (64 scenes): at 8 scenes the 25 MB of a call are 5 us of HBM
    # time, below two launch latencies, so the bandwidth fraction at B = 8 measures launch-sized kernels; B = 64 is
    # the size at which the operator can be judged against the HBM roofline at all
    bq64 = None
    if rank == 0 and world == 1 and kind == "model" and not dry and not args.no_extras and args.full:
        with torch.no_grad():
            big = torch.cat([make_batch_t(B_PER_GPU, N_POINTS, 777 + j, dev) for j in range(8)], 0)
            inds = _ext.furthest_point_sampling(big, M_CENTRES)
            new_big = torch.gather(big, 1, inds.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
            t64 = _ext.enable_kernel_timing(["query_and_group_xyz"])
            for _ in range(3 + args.steps):
                torch.cuda.synchronize()
                _ext.query_and_group_xyz(new_big, big, RADIUS, NSAMPLE, True, channels_last=True)
            torch.cuda.synchronize()
            _ext.disable_kernel_timing()
        ev = t64.get("query_and_group_xyz", [])[3:]
        if ev:
            ms64 = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
            by = BQ_GROUP_BYTES_PER_SCENE * 64
            bq64 = {"kernel": "grid_build_kernel + grid_query8_kernel, B = 64 scenes in one call (the global batch on one "
                              "GPU), GPU otherwise idle",
                    "timing": "HIP events around each call", "bound": "hbm", "achieved": round(by / (ms64 * 1e-3) / 1e9, 3),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(by / (ms64 * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                    "traffic": None, "bytes_per_launch": by, "avg_launch_ms": round(ms64, 5)}
        del big, new_big

    if rank == 0:
        bq_ms = avg_ms("query_and_group_xyz") or avg_ms("ball_query")
        bq_alone_ms = avg_ms("query_and_group_xyz", alone)
        fps_ev = timing.get("furthest_point_sampling", [])
        # two FPS calls per step in the model workload (20000->2048, 2048->nq): report the large one
        fps_ms = max((s.elapsed_time(e) for s, e in fps_ev), default=None)
        bytes_per_launch = BQ_GROUP_BYTES_PER_SCENE * B_PER_GPU
        achieved = bytes_per_launch / (bq_ms * 1e-3) / 1e9 if bq_ms else None
        bq_roofline = {
            "kernel": "grid_build_kernel + grid_query8_kernel (cell-binned ball_query fused with xyz grouping, "
                      "one coda_query_and_group_xyz_f32 call)",
            "timing": ("HIP events around each call inside the timed region"
                       + (" (side stream, concurrent with the step's kernels)" if prefetch else "")),
            "bound": "hbm",
            "achieved": round(achieved, 3) if achieved else None,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 5) if achieved else None,
            # HBM bytes per launch from PMC (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE), separate rocprofv3 --pmc passes
            # of tools/bench_ops.py on THIS round's kernels (tools/pmc_bq.sh): build 1089.0 KB x2 + 3012.2 KB, query
            # 2666.0 KB x2 + 16384.0 KB -- profiles/r05_pmc_ball_query.md (not collected in this run)
            "traffic": BQ_TRAFFIC_PMC,
            "traffic_source": "profiles/r05_pmc_ball_query.md",
            "bytes_per_launch": bytes_per_launch,
            "avg_launch_ms": round(bq_ms, 5) if bq_ms else None,
            # same operator, same inputs, GPU otherwise idle (only reported when the timed region ran it
            # concurrently with the step on a side stream)
            "avg_launch_ms_alone": round(bq_alone_ms, 5) if bq_alone_ms else None,
            "frac_alone": round(bytes_per_launch / (bq_alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
            if bq_alone_ms else None,
        }

        # Round 6: the long-sequence backward (l, s >= 1024, whole tiles, head width 64: the encoder's launches) runs
        # part of its products on the bf16 matrix cores with three-piece operands -- six bf16 products per fp32 product,
        # 2500 / 6 = 416.7 TFLOP/s-equivalent.  Units of (Lq * Lk * 256 * scenes * 2 flops) on that pipe per kind:
        x3_dkv = os.environ.get("CODA_ATTN_DKV_X3", "1") != "0"
        x3_dq = any(k[0] == "ktp" for k in attn_ms_all) or any(k[0] == "ktp" for k in attn_ms)
        x3_fwd = os.environ.get("CODA_ATTN_FWD_X3", "1") != "0"  # the encoder's forward: the fused core's three-piece mode
        MFMA_X3_PEAK = MFMA_BF16_PEAK_TFLOPS / 6.0

        def x3_units(k, l, s_len):
            if l < 1024 or s_len < 1024 or l % 32 or s_len % 32:
                return 0
            return {"dkv": 4 if x3_dkv else 0, "dqg": 2 if x3_dq else 0, "fwd": 4 if x3_fwd else 0}.get(k, 0)

        def attn_entry(key, samples, timing_note):
            k, l, s_len = key
            ms = sum(samples) / len(samples)
            flops = ATTN_FLOPS[k] * l * s_len * 256 * B_PER_GPU  # 4 heads x 64 = 256 model channels
            tf = flops / (ms * 1e-3) / 1e12
            names = {"fwd": "mha_fwd_kernel", "dkv": "mha_bwd_dkv_kernel", "dq": "mha_bwd_dq_kernel",
                     "dqg": "mha_bwd_dq_gemm_kernel", "bwdf": "mha_bwd_fused_kernel", "dqr": "mha_dq_reduce_kernel"}
            ux = x3_units(k, l, s_len)
            name = names[k]
            # the peak a launch is priced against: its products on the fp32 MFMA at 157.3 TFLOP/s, those on the
            # three-piece bf16 path at 416.7 TFLOP/s-equivalent -- the harmonic blend by units (all-fp32 launches: 157.3)
            peak = ATTN_FLOPS[k] / ((ATTN_FLOPS[k] - ux) / MFMA_F32_PEAK_TFLOPS + ux / MFMA_X3_PEAK) if ATTN_FLOPS[k] else MFMA_F32_PEAK_TFLOPS
            e = {"kernel": f"{name} (queries {l} x keys {s_len}, {B_PER_GPU} scenes x 4 heads x 64, "
                           f"dropout 0.1)",
                 "timing": timing_note, "bound": "mfma", "achieved": round(tf, 2),
                 "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                 "traffic": None, "flops_per_launch": flops,
                 "flops_formula": f"{ATTN_FLOPS[k]} * Lq * Lk * 256 * scenes = EXECUTED MFMA flops (fp32-equivalent): " + ATTN_UNITS_NOTE[k],
                 # the same launch on SURVEY 8d's algorithmic count (recomputed products not credited)
                 "frac_algorithmic": round(tf * ATTN_FLOPS_ALG[k] / ATTN_FLOPS[k] / peak, 4),
                 "avg_launch_ms": round(ms, 5), "launches": len(samples)}
            if ux:
                pipes = {"dkv": "S and dP (4 units: both operands are staged tiles) on v_mfma_f32_32x32x16_bf16 with "
                                "three-piece operands, dV and dK (4 units) on the fp32 MFMA",
                         "dqg": "the whole product on v_mfma_f32_32x32x16_bf16 with three-piece operands; the launch "
                                "streams dS (537 MB) once: see hbm_frac",
                         "fwd": "both products on v_mfma_f32_32x32x16_bf16 with three-piece operands (the probabilities are "
                                "split per element: the soft-max + split vector work bounds this launch, DESIGN.md section 4)"}[k]
                e["kernel"] = e["kernel"].replace(name, {"dkv": "mha_bwd_dkv_x3_kernel", "dqg": "mha_bwd_dq_x3_kernel",
                                                         "fwd": "mha_fwd_bf16_kernel<three pieces>"}[k])
                e["peak_note"] = (f"{ux} of {ATTN_FLOPS[k]} units at 2500 / 6 = 416.7 TFLOP/s-equivalent (six bf16 piece "
                                  f"products per fp32 product), the rest at the fp32 MFMA's 157.3: {pipes}.  Rounds 1-5 "
                                  "priced this launch against 157.3 alone (frac_of_fp32_mfma_peak keeps that reading; it is "
                                  "not bounded by 1 any more)")
                e["frac_of_fp32_mfma_peak"] = round(tf / MFMA_F32_PEAK_TFLOPS, 4)
                e["arithmetic"] = "fp32-accurate: operands split exactly into three bf16 pieces, fp32 accumulation"
            if k == "dqg":
                by = 4 * B_PER_GPU * 4 * l * s_len
                e["hbm_bytes_algorithmic"] = by + 2 * B_PER_GPU * s_len * 256 * 4
                e["hbm_frac"] = round(e["hbm_bytes_algorithmic"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            return e

        roofline, others = bq_roofline, []
        dom = ("dkv", 2048, 2048)
        if dom in attn_ms:
            roofline = attn_entry(dom, attn_ms[dom],
                                  "HIP events around each launch inside the timed region (coda_mha_timing_*, launch "
                                  "stream)" if graph is None else
                                  "the timed region replays this kernel inside a hipGraph (no per-launch events can "
                                  "be read back): HIP events around each launch (coda_mha_timing_*, launch stream) in "
                                  "`steps` eagerly enqueued steps of the same workload right after it")
            # HBM bytes per launch from PMC (separate FETCH_SIZE / WRITE_SIZE passes), not collected in this run
            # (which backward route ran -- through the dS workspace or not -- is seen in the extra steps of --full)
            if attn_ms_all:
                via_ds = ("dqg", 2048, 2048) in attn_ms_all
                roofline["traffic"] = ATTN_DKV_TRAFFIC_DS if via_ds else ATTN_DKV_TRAFFIC
                roofline["traffic_source"] = ("profiles/r06_pmc_attention_hbm.md" if via_ds else "profiles/r03_pmc_attention_hbm.md") + \
                    " (PMC, separate FETCH_SIZE / WRITE_SIZE passes)"
                if via_ds:
                    roofline["traffic_algorithmic"] = 5 * 16_777_216 + 536_870_912 + 2 * 16_777_216  # Q K V dO O in; dS dK dV out
            # the part sustains 2.16 GHz under matrix load (tools/mfma_lds_probe.hip): what the nominal-clock peak becomes
            roofline["frac_of_sustained_clock_peak"] = round(roofline["achieved"] / (roofline["peak"] * 2.16 / 2.4), 4)
            if attn_ms_all:  # --full
                # (dK/dV from the timed region; delta and dQ from the extra steps when the timed region recorded dK/dV only)
                bwd_kinds = ("delta", "dkv", "dq", "dqg", "ktp")
                src = {k: (attn_ms if (k, 2048, 2048) in attn_ms else attn_ms_all) for k in bwd_kinds}
                t_bwd = sum(sum(src[k][(k, 2048, 2048)]) / len(src[k][(k, 2048, 2048)])
                            for k in bwd_kinds if (k, 2048, 2048) in src[k])
                # the encoder layer's whole attention backward (delta + dK/dV + dQ launches): what it EXECUTES (dK/dV 8 + dQ
                # GEMM 2 = 10 units of Lq * Lk * d through the dS workspace, 14 in the two-kernel form) and SURVEY 8d's
                # algorithmic 8.  (Rounds 4-5 printed `frac_whole_backward_8d` with 12 units credited -- more than either.)
                # priced like the single launches: the units on the three-piece bf16 path at 416.7, the others at 157.3
                n_exec = 10 if via_ds else 14
                n_x3 = (x3_units("dkv", 2048, 2048) + x3_units("dqg", 2048, 2048)) if via_ds else 0
                peak_bwd = n_exec / ((n_exec - n_x3) / MFMA_F32_PEAK_TFLOPS + n_x3 / MFMA_X3_PEAK)
                unit = 2048 * 2048 * 256 * B_PER_GPU / (t_bwd * 1e-3) / 1e12 / peak_bwd
                roofline["frac_whole_backward_executed"] = round(n_exec * unit, 4)
                roofline["frac_whole_backward_algorithmic"] = round(8 * unit, 4)
                roofline["whole_backward_peak_tflops"] = round(peak_bwd, 1)
                roofline["whole_backward_ms"] = round(t_bwd, 5)
            note = "HIP events around each launch, `steps` extra steps right after the timed region"
            for key in sorted(attn_ms_all, key=lambda k: (-k[1] * k[2], k[0])):
                if key[0] not in ("delta", "dqr", "ktp") and key != dom:
                    others.append(attn_entry(key, attn_ms_all[key], note))
            # the six decoder-shaped kernels together (north_star: >= 50 % of the MFMA peak on decoder attention):
            # sum of the flops of one launch of each / sum of their event-timed durations
            # (every launch of the two shapes counts, the stand-alone rowsum(dO * O) and the partial-tile sum of the
            # one-kernel backward included: they are part of the time, not of the flops)
            dec_keys = [k for k in attn_ms_all if k[1] == 256 and k[2] in (256, 2048)]
            if dec_keys:
                fl = sum(ATTN_FLOPS[k[0]] * k[1] * k[2] * 256 * B_PER_GPU for k in dec_keys)
                ms = sum(sum(attn_ms_all[k]) / len(attn_ms_all[k]) for k in dec_keys)
                # SURVEY 8d's ALGORITHMIC count: forward 4 + backward 8 (+4 for one recomputation of S) = 16 units of
                # Lq * Lk * d per shape; the two-kernel backward EXECUTES 14 (S recomputed in both kernels) = 18 with
                # the forward.  Both fractions are reported; the north-star bar is read on the algorithmic one.
                shapes = sorted({(k[1], k[2]) for k in dec_keys})
                fl_alg = sum(16 * l * s_len * 256 * B_PER_GPU for l, s_len in shapes)
                others.append({"kernel": "decoder_aggregate: cross-attention (256 x 2048) and self-attention (256 x 256), "
                                         "forward + whole backward, one launch of each kernel: "
                                         + ", ".join(f"{k[0]}_{k[1]}x{k[2]}" for k in sorted(dec_keys, key=lambda k: (-k[2], k[0]))),
                               "timing": note, "bound": "mfma", "achieved": round(fl_alg / (ms * 1e-3) / 1e12, 2),
                               "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(fl_alg / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                               "frac_algorithmic": round(fl_alg / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                               "frac_executed": round(fl / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4), "traffic": None,
                               # forward 4 + backward 8 and nothing for any recomputation (12 units per shape)
                               "frac_no_recompute_credit": round(0.75 * fl_alg / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                               "flops_algorithmic": fl_alg, "flops_executed": fl,
                               "flops_formula": "algorithmic: 16 * Lq * Lk * 256 * scenes per shape (SURVEY 8d: fwd 4, bwd 8 "
                                                "+ 4 recomputed -- the count VERDICT r5 applied); executed: fwd 4 + (dK/dV 8 + dQ 6 "
                                                "| one-kernel backward 10: S recomputed once, so executed < SURVEY's 16)",
                               "sum_launch_ms": round(ms, 5), "kernels": len(dec_keys)})
            # the set-abstraction MLP's hand-written fp32-MFMA GEMM kernels (csrc/sa_mfma.hip): 2 * rows * Cin * Cout
            # flops per launch over the packed (de-duplicated) rows of the step's 8 scenes
            if sa_ms and sa_rows:
                rows = sum(sa_rows) / len(sa_rows)
                names = {"fwd2": ("sa_fwd_kernel<64,128> (layer 2: layer 1 recomputed from xyz + BN + ReLU prologue, "
                                  "statistics epilogue)", 64, 128),
                         "fwd3": ("sa_fwd_kernel<128,256> (layer 3: BN + ReLU prologue, statistics + max-pool "
                                  "epilogue)", 128, 256),
                         "dx3": ("sa_bwd_dx_kernel<128,256> (dy3 from the pooled gradient on the fly, dA2 + ReLU mask + "
                                 "BN sums)", 128, 256),
                         "dw3": ("sa_bwd_dw_kernel<128,256> + partial-tile reduction (dW3 = dy3^T a2)", 128, 256),
                         "dx2": ("sa_bwd_dx_kernel<64,128> (dA1 + layer 1's sums in the epilogue)", 64, 128),
                         "dw2": ("sa_bwd_dw_kernel<64,128> + partial-tile reduction", 64, 128)}
                tot_fl, tot_ms = 0.0, 0.0
                for key, (label, cin, cout) in names.items():
                    if key in sa_ms:
                        fl = 2.0 * rows * cin * cout
                        tf = fl / (sa_ms[key] * 1e-3) / 1e12
                        tot_fl += fl
                        tot_ms += sa_ms[key]
                        others.append({"kernel": label, "timing": note, "bound": "mfma", "achieved": round(tf, 2),
                                       "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                       "frac": round(tf / MFMA_F32_PEAK_TFLOPS, 4), "traffic": None,
                                       "flops_per_launch": int(fl), "flops_formula": "2 * packed rows * Cin * Cout",
                                       "packed_rows": int(rows), "avg_launch_ms": round(sa_ms[key], 5)})
                if tot_ms:
                    tf = tot_fl / (tot_ms * 1e-3) / 1e12
                    others.append({"kernel": "sa_mlp_aggregate: the six MFMA GEMM launches of the shared MLP, forward + backward",
                                   "timing": note, "bound": "mfma", "achieved": round(tf, 2), "peak": MFMA_F32_PEAK_TFLOPS,
                                   "unit": "TFLOP/s", "frac": round(tf / MFMA_F32_PEAK_TFLOPS, 4), "traffic": None,
                                   "flops": int(tot_fl), "sum_launch_ms": round(tot_ms, 5)})
            others.append(bq_roofline)
            if bq64 is not None:
                others.append(bq64)
        # The kernel figures BASELINE.json's metric and north_star name next to the scenes/s, as SCALARS inside `roofline`
        # (and copied into `config`): the driver's parsed record keeps these two objects whole, while `roofline_others`
        # is dropped from it and cut from the stdout tail (missing 1).
        def _find(prefix):
            return next((o for o in others if o["kernel"].startswith(prefix)), None)

        north_star = {
            "ball_query_group_bytes_algorithmic": bytes_per_launch,  # 8 scenes x 3 126 016 B
            "ball_query_group_traffic_pmc": BQ_TRAFFIC_PMC if bq_ms else None,
            "ball_query_group_us_in_step": round(bq_ms * 1e3, 2) if bq_ms else None,
            "ball_query_group_GBps_in_step": bq_roofline["achieved"],
            "ball_query_group_frac_in_step": bq_roofline["frac"],
            "ball_query_group_us_alone": round(bq_alone_ms * 1e3, 2) if bq_alone_ms else None,
            "ball_query_group_GBps_alone": round(bytes_per_launch / (bq_alone_ms * 1e-3) / 1e9, 1) if bq_alone_ms else None,
            "ball_query_group_frac_alone": bq_roofline["frac_alone"],
        }
        if bq64 is not None:
            north_star.update(ball_query_group_B64_us=round(bq64["avg_launch_ms"] * 1e3, 2),
                              ball_query_group_B64_GBps=bq64["achieved"], ball_query_group_B64_frac=bq64["frac"],
                              ball_query_group_B64_bytes_algorithmic=bq64["bytes_per_launch"])
        dec = _find("decoder_aggregate")
        if dec is not None:
            north_star.update(decoder_attention_frac_algorithmic=dec["frac_algorithmic"],
                              decoder_attention_frac_executed=dec["frac_executed"],
                              decoder_attention_frac_no_recompute_credit=dec["frac_no_recompute_credit"],
                              decoder_attention_units="algorithmic 16 per shape (SURVEY 8d: fwd 4 + bwd 8 + 4 recomputed), "
                                                      "executed 14 (one-kernel backward: S recomputed once), 12 without any "
                                                      "recomputation credit; time = every launch of the two shapes",
                              decoder_attention_TFLOPs_algorithmic=dec["achieved"],
                              decoder_attention_us=round(dec["sum_launch_ms"] * 1e3, 2),
                              decoder_attention_launches=dec["kernels"])
        sa_agg = _find("sa_mlp_aggregate")
        if sa_agg is not None:
            north_star.update(sa_mlp_frac=sa_agg["frac"], sa_mlp_us=round(sa_agg["sum_launch_ms"] * 1e3, 2))
        if fps_ms:
            north_star["fps_20000_to_2048_ms"] = round(fps_ms, 4)
        if roofline is not bq_roofline:
            roofline["north_star"] = north_star
        out = {
            "metric": "scenes/sec fwd+bwd (20k pts, 256 queries)",
            "value": round(world * B_PER_GPU * args.steps / dt, 3),
            "unit": "scenes/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": desc, "scenes_per_gpu": B_PER_GPU, "points": N_POINTS,
                       "parallelism": f"dp{world}" + ("" if world == 1 and not force_ddp else
                                                          " (flat gradient all-reduce)" if reducer is not None else " (torch DDP)"),
                       "optimizer": "clip_grad_norm_(0.1) + AdamW, in the timed region (engine.py:161-164)",
                       "execution": ("set-abstraction stage eager; encoder + decoder + heads + loss, forward and "
                                     "backward, replayed as one hipGraph; optimizer eager"
                                     if graph is not None else "eager"),
                       "sampling": ("FPS + ball query of batch i+1 run on a side stream during step i (once per "
                                    "step, inside the timed region); padded group copies are computed once"
                                    if prefetch else "in line"),
                       "library_gemms": "the libraries' own heuristics (no tuning table)",
                       # which arithmetic the products of the step run on ("dtype": "f32" = every tensor is fp32 and every
                       # result is fp32-ACCURATE: the bf16x3 routes are closer to float64 than the fp32 library GEMM,
                       # tests/test_gemm_x3_gpu.py, tools/x3_error.py)
                       "arithmetic": _arithmetic_note()},
            "roofline": roofline,
            # host side of the timed region on rank 0: time until the last step was enqueued (close to the wall
            # time when the host is the bottleneck -- or when the GPU is and the launch queue fills up) and what
            # Python's garbage collector took of it
            "host": {"enqueue_ms_per_step": round(t_host / args.steps * 1e3, 4), "settle_steps": settle_steps,
                     "settle_s": round(settle_s, 2),
                     "slack_probe_ms": round(slack_probe_ms, 3) if slack_probe_ms is not None else None,
                     "wait_s": host_wait_s,
                     "gc_passes": gc_stat["n"], "gc_ms_per_step": round(gc_stat["ms"] / args.steps, 4)},
            "kernels_ms": {"furthest_point_sampling_20000_to_2048": round(fps_ms, 4) if fps_ms else None},
        }
        for k_ns in ("ball_query_group_GBps_in_step", "ball_query_group_GBps_alone", "ball_query_group_B64_GBps",
                     "ball_query_group_B64_frac", "decoder_attention_frac_algorithmic", "decoder_attention_frac_executed"):
            if north_star.get(k_ns) is not None:
                out["config"][k_ns] = north_star[k_ns]
        if unchanged is not None:
            out["config"]["value_unchanged"] = unchanged["value"]  # (also inside config: the driver's parsed record keeps it)
            out["value_unchanged"] = unchanged["value"]
            out["ms_per_step_unchanged"] = unchanged["ms_per_step"]
            out["value_unchanged_caller"] = unchanged
        out["comm"] = comm
        if others:
            # aggregates and the ball-query operator first, single kernels behind them (a reader of a truncated line
            # sees the figures the north-star bars are read on)
            lead = [o for o in others if o["kernel"].startswith(("decoder_aggregate", "sa_mlp_aggregate", "grid_build_kernel"))]
            out["roofline_others"] = lead + [o for o in others if o not in lead]
        if world == 1 and not dry and not args.no_extras and kind == "model" and args.workload != "model40k" and args.full:
            # extra keys, measured by this same command right after the headline (fewer steps: they are
            # secondary lines; the headline's timed region above is untouched by them)
            ex_steps, ex_warm = max(5, min(args.steps, 10)), 3
            out["extra_configs"] = {"configs[1]_sa_only": run_extra("sa", dev, ex_steps, ex_warm),
                                    "configs[1]_sa_only_sampling_ahead": run_extra("sa_prefetch", dev, ex_steps, ex_warm),
                                    "configs[4]_40k_512q_bf16_one_gpu": run_extra("model40k", dev, ex_steps, ex_warm),
                                    "scripts_variant_dec512_128q": run_extra("scripts", dev, ex_steps, ex_warm),
                                    "clip_image_tower": run_image_tower(dev, ex_steps, ex_warm),
                                    "alignment_loss_stage2_classes": run_alignment_extra(dev),
                                    "configs[2]_with_image_branch": run_extra("distill", dev, ex_steps, ex_warm)}
        if world == 1 and not args.no_cpu_baseline and not dry and args.full:
            out["cpu_baseline"] = cpu_baseline(kind)
        if (world == 1 and not dry and unchanged is not None and ("extra_configs" in out or "cpu_baseline" in out)
                and os.environ.get("CODA_BENCH_UNCHANGED_REPEAT", "1") != "0"):
            # The unchanged caller once more, at the END of the run (same loop, same step count).  Its host side is the
            # heavier one (torch's optimizer and clip, a blocking .item() per step: host time adds to GPU time), so a box
            # that is still busy with its own start-up shows here first: the first process on a fresh box read 348-358
            # scenes/s where every later process of the same box read 491-498 (tools/ab_default.sh; the headline leg
            # waits such a phase out with its slack probe, this leg cannot -- it is host-serialised by construction).
            # Both readings stay in the record with their time since process start; the steady-state figure is the
            # larger one.
            dt3 = time_unchanged()
            again = round(world * B_PER_GPU * args.steps / dt3, 3)
            unchanged["readings"] = [{"value": unchanged["value"], "at_s": round(unchanged_at_s, 1)},
                                     {"value": again, "at_s": round(time.perf_counter() - T_PROCESS_START, 1)}]
            if again > unchanged["value"]:
                unchanged["value"] = again
                unchanged["ms_per_step"] = round(dt3 / args.steps * 1e3, 4)
            out["config"]["value_unchanged"] = out["value_unchanged"] = unchanged["value"]
            out["ms_per_step_unchanged"] = unchanged["ms_per_step"]
        if dumped is not None:
            out["dump_outputs"] = dumped
        if dry:
            out.update(metric="dry run (control flow only)", data="none", dtype="f32")
        line = compact_line(out, dry)
    else:
        line = None
    if dist.is_initialized():
        dist.destroy_process_group()  # RCCL prints its version banner to stdout here: the JSON line goes after it
    if line is not None:
        sys.stdout.flush()
        print(line, flush=True)


if __name__ == "__main__":
    main()
