"""The sequence of `ops` calls of every transformer-tower pass, recorded without a GPU:

    python tests/golden/make_golden_tower_trace.py          # writes tests/golden/tower_call_trace.json

Every `ops` function the tower passes and their backwards call is replaced (setattr on the module: the passes look `ops.<name>` up at call time) by a stub
that returns CPU tensors of the real function's dtypes and shapes, honours `out=`, and appends one line: the op and its arguments, bound through the real
function's signature with defaults applied (positional / keyword spelling does not matter).  A tensor is written as dtype, shape, strides when not
contiguous, and where its storage came from — a parameter's name, `input`, `#i` for the i-th call of the case (`#i.k`: its k-th output), `host<k>` for
the k-th storage torch itself produced (a cached cast, a clone, a zero-filled buffer) — plus the storage offset: the trace pins data flow and aliasing,
not only shapes.  The cases are tests/tower_pass_cases.py; they use public entry points only, so this file records the same thing on any commit."""
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tower_pass_cases  # noqa: E402

OUT = os.path.join(HERE, "tower_call_trace.json")
F16, F32 = torch.float16, torch.float32


def _z(*shape, dtype=F16):
    return torch.zeros(*shape, dtype=dtype)


def _ln_rows(a):
    D = a["x"].shape[-1]
    return a["out"] if a["out"] is not None else _z(a["x"].numel() // D if a["rows"] is None else a["rows"], D)


def _ln_backward(a):
    D = a["x"].shape[-1]
    sums = _z(2 * D, dtype=F32)
    return torch.zeros_like(a["x"]), sums[:D], sums[D:]


def _im2col(a):
    B, _, R, _ = a["img"].shape
    G, P = R // a["P"], a["P"]
    return _z(B * G * G, (3 * P * P + 63) // 64 * 64)


def _prompt_ctx_grad(a):
    W = a["dx"].shape[1]
    return _z(*((a["N"], a["n_ctx"], W) if a["class_specific"] else (a["n_ctx"], W)), dtype=F32)


def _couple_backward(a):
    (depth, P, Wt), Wv = a["x"].shape, a["weight"].shape[1]
    return (_z(depth, P, Wt, dtype=F32) if a["want_x"] else None, _z(depth, Wv, Wt, dtype=F32) if a["want_weight"] else None,
            _z(depth, Wv, dtype=F32) if a["want_bias"] else None)


def _vit_embed_backward(a):
    W = a["dt"].shape[-1]
    return (_z(a["L"], W, dtype=F32) if a["want_pos"] else None, _z(a["B"] * (a["L"] - 1), W) if a["want_patch"] else None)


def _text_embed_backward(a):
    W = a["dx"].shape[-1]
    return (_z(a["vocab"], W, dtype=F32) if a["want_emb"] else None, _z(a["tokens"].shape[1], W, dtype=F32) if a["want_pos"] else None)


# name -> what the stub returns, from the bound arguments (the shapes and dtypes proto_clip_amd/ops.py allocates)
STUBS = {
    "gemm": lambda a: a["out"] if a["out"] is not None else _z(a["a"].shape[0], a["w"].shape[0]),
    "layernorm": _ln_rows,
    "add_layernorm": _ln_rows,
    "attention": lambda a: a["out"] if a["out"] is not None else _z(a["B"] * a["L"], a["H"] * 64),
    "attention_first_queries": lambda a: _z(a["B"] * a["Lq"], a["H"] * 64),
    "im2col_patches": _im2col,
    "vit_embed_ln": lambda a: (_z(a["B"] * (a["G2"] + 1), a["W"]), _z(a["B"] * (a["G2"] + 1), a["W"])),
    "vit_assemble_tokens": lambda a: _z(a["B"] * (a["G2"] + 1), a["W"]),
    "text_embed": lambda a: _z(a["tokens"].numel(), a["tok_emb"].shape[1]),
    "gather_eot": lambda a: _z(a["B"], a["W"]),
    "prompt_embed": lambda a: _z(a["tokens"].shape[0] * (a["tokens"].shape[1] if a["L_out"] is None else a["L_out"]), a["tok_emb"].shape[1]),
    "prompt_ctx_grad": _prompt_ctx_grad,
    "vpt_append": lambda a: _z(a["B"] * (a["L0"] + a["ctx"].shape[0]), a["ctx"].shape[-1]),
    "vpt_replace_": lambda a: a["x"],
    "vpt_grad": lambda a: _z(a["P"], a["g"].shape[1], dtype=F32),
    "rows_replace_": lambda a: a["x"],
    "rows_grad": lambda a: _z(a["P"], a["g"].shape[1], dtype=F32),
    "couple": lambda a: _z(a["x"].shape[0], a["x"].shape[1], a["weight"].shape[1], dtype=F32),
    "couple_backward": _couple_backward,
    "transpose": lambda a: _z(a["x"].shape[1], a["x"].shape[0]),
    "cast_f16": lambda a: _z(*a["x"].shape),
    "colsum_f16": lambda a: _z(a["x"].shape[1], dtype=F32),
    "quick_gelu_backward": lambda a: torch.zeros_like(a["u"]),
    "layernorm_backward_f32": _ln_backward,
    "attention_backward": lambda a: torch.zeros_like(a["qkv"]),
    "vit_embed_backward": _vit_embed_backward,
    "text_embed_backward": _text_embed_backward,
}

DTYPES = {torch.float16: "f16", torch.float32: "f32", torch.int64: "i64", torch.float64: "f64"}


class Recorder:
    """The lines of one case.  Every tensor seen is kept alive until the case ends, so a storage address names one storage."""

    def __init__(self):
        self.lines, self.labels, self.keep, self.n_host = [], {}, [], 0

    def name(self, named):
        for label, t in named.items():
            self.keep.append(t)
            self.labels.setdefault(t.untyped_storage().data_ptr(), label)

    def describe(self, v):
        if isinstance(v, torch.Tensor):
            self.keep.append(v)
            key = v.untyped_storage().data_ptr()
            if key not in self.labels:
                self.labels[key] = f"host{self.n_host}"
                self.n_host += 1
            strides = "" if v.is_contiguous() else "/" + ",".join(map(str, v.stride()))
            return f"{DTYPES.get(v.dtype, v.dtype)}[{','.join(map(str, v.shape))}]{strides}@{self.labels[key]}+{v.storage_offset()}"
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.describe(x) for x in v) + ")"
        return repr(v)

    def stub(self, name, real):
        sig = inspect.signature(real)

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            index = len(self.lines)
            self.lines.append(f"{name}(" + ", ".join(f"{k}={self.describe(v)}" for k, v in bound.arguments.items()) + ")")
            with torch.no_grad():
                out = STUBS[name](bound.arguments)
            tensors = [t for t in (out if isinstance(out, tuple) else (out,)) if t is not None]
            for k, t in enumerate(tensors):
                self.keep.append(t)
                self.labels.setdefault(t.untyped_storage().data_ptr(), f"#{index}" if len(tensors) == 1 else f"#{index}.{k}")
            return out
        return call


def record(run):
    """The trace of one case of tower_pass_cases.cases()."""
    from proto_clip_amd import ops
    rec = Recorder()
    real = {name: getattr(ops, name) for name in STUBS}
    try:
        for name, fn in real.items():
            setattr(ops, name, rec.stub(name, fn))
        run("cpu", rec.name)
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)
    return rec.lines


def record_all():
    return {key: record(run) for key, run in tower_pass_cases.cases().items()}


if __name__ == "__main__":
    traces = record_all()
    with open(OUT, "w") as fh:
        json.dump(traces, fh, indent=0)
        fh.write("\n")
    print(f"{OUT}: {len(traces)} cases, {sum(map(len, traces.values()))} calls")
