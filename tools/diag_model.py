#!/usr/bin/env python3
"""Diagnostic: tiny-model forward/backward error vs the golden fixture, with the fused
attention core and with the torch fp32 reference core (GPU), to localise numerical drift."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from golden import parts as golden_parts  # noqa: E402
from golden.weights import fill_deterministic, grad_digest  # noqa: E402
from test_model_structure import tiny_args  # noqa: E402

from coda_neurips2023_amd import attention_core  # noqa: E402
from coda_neurips2023_amd.dataset_config import HotPathDatasetConfig  # noqa: E402
from coda_neurips2023_amd.model_3detr import build_model  # noqa: E402
from oracle.cpu_port import attention_ref  # noqa: E402

G = golden_parts.load("model_tiny.npz")
dev = torch.device("cuda:0")


def run(tag):
    model, _ = build_model(tiny_args(), HotPathDatasetConfig())
    fill_deterministic(model, seed=9)
    model.to(dev).train()
    inputs = {"point_clouds": torch.from_numpy(G["pc"]).to(dev),
              "point_cloud_dims_min": torch.from_numpy(G["dims_min"]).to(dev),
              "point_cloud_dims_max": torch.from_numpy(G["dims_max"]).to(dev)}
    pred = model(inputs)
    o = pred["outputs"]
    errs = []
    for k in [f for f in G.files if f.startswith("train_out/")]:
        name = k.split("/", 1)[1]
        ref = G[k]
        errs.append((float(np.abs(o[name].detach().cpu().numpy() - ref).max() / (np.abs(ref).max() + 1e-12)), name))
    print(tag, "forward worst:", sorted(errs, reverse=True)[:4])
    loss = 0
    for name in ["sem_cls_logits", "text_correlation_embedding", "center_normalized", "size_normalized",
                 "angle_logits", "angle_residual", "box_corners"]:
        w = torch.from_numpy(G[f"train_lossw/{name}"]).to(dev)
        loss = loss + (o[name] * w).sum()
        for aux in pred["aux_outputs"]:
            loss = loss + 0.5 * (aux[name] * w).sum()
    loss.backward()
    dig = grad_digest(model)
    gmax = max(G[k][1] for k in G.files if k.startswith("train_grad/"))
    worst = []
    for k in [f for f in G.files if f.startswith("train_grad/")]:
        n = k.split("/", 1)[1]
        ref = G[k]
        worst.append((float(np.abs(dig[n][2:] - ref[2:]).max() / max(np.abs(ref[2:]).max(), 1e-4 * gmax)), n, float(ref[1])))
    worst.sort(reverse=True)
    print(tag, "loss", float(loss), float(G["train_loss"]))
    print(tag, "grad worst:", worst[:8])


os.environ["CODA_SA_MLP"] = "fused"
run("fused-SA  fused-attn")
os.environ["CODA_SA_MLP"] = "layers"
run("layers-SA fused-attn")
attention_core.attention = attention_ref
run("layers-SA torch-attn")
