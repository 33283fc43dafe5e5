#!/usr/bin/env python3
"""Generates tests/golden/adapter_shapes.npz by RUNNING THE REFERENCE ITSELF, through make_golden.py's import shim: the reference's own
`model.Adapter(D, c_type, width=W, dtype=torch.half)` and `model.Adapter_FC(D, reduction=r, dtype=torch.half)` on the CPU, at the widths /
reductions / feature dims beyond `Adapter(D, kind)` / `Adapter_FC(D)` at D % 256 == 0.  Per case: the state-dict key list, the parameter
shapes and the reference's fp16 output rows.  Outputs and seeds only: a test regenerates the weights through the product's own module
(`torch.manual_seed(seed)`, construct, `spec.randomize_adapter_(ad, seed)`: the same draws in the same order) and the unit rows from the stored seed.

    python tests/golden/make_golden_adapter_shapes.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
from proto_clip_amd import synth                                   # noqa: E402
from spec import randomize_adapter_                                 # noqa: E402

ROWS, ROW_SEED = 16, 3        # 16 rows per case: fp16 noise does not compress, and 31 cases of them are 0.7 MB
CONV_CASES = [(kind, W, D) for kind in ("conv-3x", "conv-2x") for W in (8, 24, 32) for D in (512, 640, 768, 1024)]
CONV_CASES += [("conv-3x", 32, 200), ("conv-3x", 32, 577)]     # partial last pixel tile; s = 25, 625 pixels
FC_CASES = [(640, 4), (640, 2), (768, 8), (512, 16), (1024, 32)]


# The one new shape the reference's main.py reaches by itself: `adapter: fc` at RN50x4's D = 640.  A spec.TRAIN-style tuple
# (N, K, D, Qv, Qt, alpha, beta, kind, sigma, vis_only, losses, epochs, lr); it lives here and in tests/test_gpu_adapter_shapes.py, not in spec.py.
TRAIN_FC_640 = ("T_fc_640", (6, 4, 640, 48, 48, 0.4, 6.0, "fc", 5.0, False, ["L1", "L2", "L3"], 2, 0.001))


def case_tag(kind, a, D):
    return f"{kind}_w{a}_d{D}" if kind != "fc" else f"fc_r{a}_d{D}"


def case_seed(index):
    return 100 + index


def unit_rows(D):
    return synth.make_split(4, 4, D, 4, 4, seed=ROW_SEED).visual_memory_keys.t().contiguous()[:ROWS]     # [16, D] fp16 unit rows


def main():
    ref_model = mg.import_reference()[2]
    out = {"rows": ROWS, "row_seed": ROW_SEED}
    tags = []
    cases = [(k, W, D) for k, W, D in CONV_CASES] + [("fc", r, D) for D, r in FC_CASES]
    for i, (kind, a, D) in enumerate(cases):
        seed = case_seed(i)
        torch.manual_seed(seed)
        ad = ref_model.Adapter_FC(D, reduction=a, dtype=torch.half) if kind == "fc" else ref_model.Adapter(D, kind, width=a, dtype=torch.half)
        randomize_adapter_(ad, seed)
        with torch.no_grad():
            y = ad(unit_rows(D))
        assert y.dtype == torch.float16 and torch.isfinite(y.float()).all()
        tag = case_tag(kind, a, D)
        tags.append(tag)
        sd = ad.state_dict()
        out[tag + "__seed"] = seed
        out[tag + "__keys"] = np.array(list(sd.keys()))
        out[tag + "__shapes"] = np.array([",".join(str(n) for n in v.shape) for v in sd.values()])
        out[tag + "__out"] = y
    out["tags"] = np.array(tags)
    mg.savez("adapter_shapes", **out)


def main_train(ref_main, ref_utils, scratch):
    """tests/golden/train_T_fc_640.npz: make_golden.make_train (the reference's own training loop, main.py:216-381) on the case above, then cut down —
    the adapter alone is 205 k parameters, so of make_train's record this keeps the episodes' labels and loss terms of EVERY step, the validation accuracies,
    and the gradients / updated parameters of the FIRST optimizer step.  The initial state is not stored: the banks are the split's, and the adapter is what
    `torch.manual_seed(1); nn.Embedding(N * K, D); Adapter_FC(D, dtype=torch.half)` draws (the reference's order, main.py:110-117) — checked here."""
    import spec
    name, case = TRAIN_FC_640
    spec.TRAIN[name] = case                                          # in this process only
    mg.make_train(name, ref_main, ref_utils, scratch)
    path = os.path.join(HERE, "train_" + name + ".npz")
    full = dict(np.load(path))
    from proto_clip_amd.model import Adapter_FC
    N, K, D = case[:3]
    torch.manual_seed(1)
    torch.nn.Embedding(num_embeddings=N * K, embedding_dim=D)
    for k, v in Adapter_FC(D, dtype=torch.half).state_dict().items():
        assert np.array_equal(full["init__" + k], v.numpy()), k
    split, _ = spec.train_inputs(name)
    assert np.array_equal(full["init__visual"], split.visual_memory_keys.t().numpy()) and np.array_equal(full["init__textual"], split.textual_memory_bank.t().numpy())
    keep = {k: v for k, v in full.items() if not k.startswith(("init__", "grad1__", "grad2__", "after1__", "after2__", "final__"))}
    mg.savez("train_" + name, **keep)


if __name__ == "__main__":
    refs = mg.import_reference()
    main_train(refs[0], refs[1], refs[5])
    main()
