#!/usr/bin/env python3
"""Generates loss_ssim.npz by IMPORTING THE REFERENCE'S OWN utils/loss_utils.py (only possible where /root/reference
exists; the fixture itself is committed).

For every case of tests/loss_helpers.py (seeded image pairs, textured and flat) the file holds
    <case>/x, <case>/y    the float32 inputs
    <case>/l1             the reference's l1_loss(x, y)                             float32, CPU
    <case>/ssim           the reference's ssim(x, y)
    <case>/loss           (1 - 0.2) * l1_loss + 0.2 * (1 - ssim), the loss line of the reference's trainers
                          (gaussiansplatting/train.py:89, train_from_mesh.py:136)
    <case>/grad           d loss / d x from the reference's own autograd
-> pins tests/loss_helpers.py's float64 restatement, and its distance from float64 is the bar of tests/test_gpu_loss.py.
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True  # the reference tree is read-only input: no __pycache__ there

import numpy as np
import torch

REF = "/root/reference/gaussiansplatting"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import loss_helpers as LH  # noqa: E402


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build():
    """name -> array, everything the fixture holds."""
    ref = load(os.path.join(REF, "utils", "loss_utils.py"), "ref_loss_utils")
    out = {}
    for case in LH.CASES:
        x, y = LH.case_inputs(case)
        a = torch.from_numpy(x).clone().requires_grad_(True)
        b = torch.from_numpy(y)
        l1, ssim = ref.l1_loss(a, b), ref.ssim(a, b)
        loss = (1.0 - LH.LAMBDA) * l1 + LH.LAMBDA * (1.0 - ssim)
        loss.backward()
        out[f"{case}/x"], out[f"{case}/y"] = x, y
        out[f"{case}/l1"] = l1.detach().numpy().astype(np.float32)
        out[f"{case}/ssim"] = ssim.detach().numpy().astype(np.float32)
        out[f"{case}/loss"] = loss.detach().numpy().astype(np.float32)
        out[f"{case}/grad"] = a.grad.numpy().astype(np.float32)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "loss_ssim.npz"), **build())
