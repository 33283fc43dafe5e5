"""Every way the package runs a transformer tower, as small seeded cases behind public entry points only (encode_image / encode_text, unfreeze,
ops.low_latency, coop.PromptLearner, vpt.VisualPromptLearner, maple.MultiModalPromptLearner): the frozen pass, the low-latency pass, heads-only training,
a taped tail behind a frozen prefix, the whole stack taped, the stem on the tape, learned text context, visual prompts, multi-modal prompts (either
tower), a tower without blocks.  Each case is a forward plus
`features.sum().backward()` wherever something requires grad and returns {"features": ..., "grad.<parameter>": ...}.

Two consumers: tests/golden/make_golden_tower_trace.py records the sequence of `ops` calls of every case on the CPU (test_tower_trace_cpu.py), and
tests/test_gpu_tower_pass.py compares the bits of every returned tensor with profiles/tower_pass_refactor.txt (the MaPLe cases:
profiles/prompt_rows_refactor.txt):

    python tests/tower_pass_cases.py --digests          # on the GPU: the `digest KEY VALUE` lines of that file"""
import contextlib
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from spec import ODD, TINY, trained_like_  # noqa: E402

SPECS = {"tiny": TINY, "odd": ODD}
N_IMG, N_TXT, N_CTX = 3, 4, 3


def make_model(kw, seed, device):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    return build_model(trained_like_(random_state_dict(seed=seed, **kw), seed)).to(device)


def make_images(kw, device):
    g = torch.Generator().manual_seed(5)
    R = kw["image_resolution"]
    return torch.randn(N_IMG, 3, R, R, generator=g).half().float().to(device)


def make_tokens(kw, device, n_ctx=0):
    """[N_TXT, 77] int64 prompts: SOT, n_ctx placeholders, 1 .. 4 name tokens, EOT (the highest id), padding."""
    g = torch.Generator().manual_seed(6)
    vocab = kw["vocab_size"]
    tokens = torch.zeros(N_TXT, kw["context_length"], dtype=torch.long)
    for i in range(N_TXT):
        n_name = 1 + i % 4
        tokens[i, 0] = vocab - 2
        tokens[i, 1:1 + n_ctx] = 1
        tokens[i, 1 + n_ctx:1 + n_ctx + n_name] = torch.randint(2, vocab - 2, (n_name,), generator=g)
        tokens[i, 1 + n_ctx + n_name] = vocab - 1
    return tokens.to(device)


def _result(feats, named):
    """features, a backward where anything asks for one, and the gradients that arrived."""
    out = {"features": feats.detach()}
    if feats.requires_grad:
        feats.sum().backward()
    for name, p in named.items():
        if p.grad is not None:
            out["grad." + name] = p.grad
    return out


def _encoder_case(spec, tower, unfreeze=None, grad=True, low_latency=False):
    def run(device, on_model=lambda named: None):
        from proto_clip_amd import ops
        kw = SPECS[spec]
        model = make_model(kw, 7, device)
        x = make_images(kw, device) if tower == "image" else make_tokens(kw, device)
        named = dict(model.named_parameters())
        on_model({**named, "input": x})
        if unfreeze is not None:
            model.unfreeze(**unfreeze)
        with torch.set_grad_enabled(grad), (ops.low_latency() if low_latency else contextlib.nullcontext()):
            feats = model.encode_image(x) if tower == "image" else model.encode_text(x)
        return _result(feats, named)
    return run


def _coop_case(class_specific, truncate, taped):
    def run(device, on_model=lambda named: None):
        from proto_clip_amd import coop
        model = make_model(TINY, 8, device)
        tokens = make_tokens(TINY, device, n_ctx=N_CTX)
        learner = coop.PromptLearner([f"class{i}" for i in range(N_TXT)], model, n_ctx=N_CTX, class_specific=class_specific, tokenized_prompts=tokens,
                                     truncate=truncate, seed=3)
        named = {**dict(model.named_parameters()), "ctx": learner.ctx}
        on_model({**named, "input": learner.tokenized_prompts})
        with torch.set_grad_enabled(taped):
            feats = learner()
        return _result(feats, named)
    return run


def _vpt_case(depth, taped):
    def run(device, on_model=lambda named: None):
        from proto_clip_amd import vpt
        model = make_model(TINY, 9, device)
        images = make_images(TINY, device)
        learner = vpt.VisualPromptLearner(model, n_ctx=N_CTX, depth=depth, seed=4)
        named = {**dict(model.named_parameters()), "ctx": learner.ctx}
        on_model({**named, "input": images})
        with torch.set_grad_enabled(taped):
            feats = learner(images)
        return _result(feats, named)
    return run


def _maple_case(depth, tower, taped):
    def run(device, on_model=lambda named: None):
        from proto_clip_amd import maple
        model = make_model(TINY, 12, device)
        images = make_images(TINY, device)
        tokens = make_tokens(TINY, device, n_ctx=N_CTX)
        learner = maple.MultiModalPromptLearner([f"class{i}" for i in range(N_TXT)], model, n_ctx=N_CTX, depth=depth, tokenized_prompts=tokens, seed=5)
        named = {**dict(model.named_parameters()), "ctx": learner.ctx, "couple_weight": learner.couple_weight, "couple_bias": learner.couple_bias}
        on_model({**named, "input": images if tower == "image" else tokens})
        with torch.set_grad_enabled(taped):
            feats = learner.image_features(images) if tower == "image" else learner.text_features()
        return _result(feats, named)
    return run


def _no_blocks_case(heads):
    def run(device, on_model=lambda named: None):
        from proto_clip_amd.clip.model import build_model, random_state_dict
        sd = random_state_dict(seed=10, **dict(TINY, vision_layers=1))           # build_model counts the blocks it is given: none
        model = build_model({k: v for k, v in sd.items() if not k.startswith("visual.transformer.")}).to(device)
        images = make_images(TINY, device)
        named = dict(model.named_parameters())
        on_model({**named, "input": images})
        if heads:
            model.unfreeze(heads=True)
        return _result(model.encode_image(images), named)
    return run


def cases(gpu_only=False):
    """{key: run(device, on_model)}.  gpu_only: without the tower that has no blocks (its bits are not part of the recorded digests)."""
    out = {}
    for spec in SPECS:
        for tower in ("image", "text"):
            for grad in (False, True):
                mode = "grad" if grad else "nograd"
                out[f"frozen.{spec}.{tower}.{mode}"] = _encoder_case(spec, tower, grad=grad)
                out[f"lowlat.{spec}.{tower}.{mode}"] = _encoder_case(spec, tower, grad=grad, low_latency=True)
            out[f"heads.{spec}.{tower}"] = _encoder_case(spec, tower, unfreeze=dict(heads=True))
            out[f"stem.{spec}.{tower}"] = _encoder_case(spec, tower, unfreeze=dict(visual_blocks=1, text_blocks=1, stem=True))
    for tower in ("image", "text"):
        out[f"tail1.tiny.{tower}"] = _encoder_case("tiny", tower, unfreeze=dict(visual_blocks=1, text_blocks=1))      # first > 0: h0 is dropped
        out[f"tail2.tiny.{tower}"] = _encoder_case("tiny", tower, unfreeze=dict(visual_blocks=2, text_blocks=2))      # first == 0: h0 enters the tail
    for specific in (False, True):
        for truncate in (True, False):
            for taped in (True, False):
                key = f"coop.tiny.{'specific' if specific else 'shared'}.{'truncated' if truncate else 'full'}.{'taped' if taped else 'nograd'}"
                out[key] = _coop_case(specific, truncate, taped)
    for depth in (1, 2):
        for taped in (True, False):
            out[f"vpt.tiny.depth{depth}.{'taped' if taped else 'nograd'}"] = _vpt_case(depth, taped)
    for depth in (1, 2):
        for tower in ("image", "text"):
            for taped in (True, False):
                out[f"maple.tiny.depth{depth}.{tower}.{'taped' if taped else 'nograd'}"] = _maple_case(depth, tower, taped)
    if not gpu_only:
        out["noblocks.tiny.image.frozen"] = _no_blocks_case(False)
        out["noblocks.tiny.image.heads"] = _no_blocks_case(True)
    return out


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def gpu_digests():
    """{"<case>/<tensor>": digest} of every tensor of every GPU case."""
    out = {}
    for key, run in cases(gpu_only=True).items():
        for name, t in run("cuda").items():
            out[f"{key}/{name}"] = digest(t)
    return out


if __name__ == "__main__":
    if sys.argv[1:] != ["--digests"]:
        raise SystemExit(__doc__)
    for k, v in gpu_digests().items():
        print("digest", k, v, flush=True)
