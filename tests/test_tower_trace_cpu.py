"""Every transformer-tower pass issues the `ops` calls recorded in tests/golden/tower_call_trace.json — the same functions in the same order on the same
operands (dtype, shape, strides, which storage at which offset), forward and backward — without a GPU: the recorder of
tests/golden/make_golden_tower_trace.py replaces the `ops` functions by shape-only stubs and the cases of tests/tower_pass_cases.py run on the CPU.
And the refusals of the taped passes stay, with their messages."""
import json

import pytest
import torch

import make_golden_tower_trace as recorder
import tower_pass_cases
from conftest import TINY

from proto_clip_amd._lib import PclipError

with open(recorder.OUT) as _fh:
    GOLDEN_TRACE = json.load(_fh)
CASES = tower_pass_cases.cases()


def test_the_golden_file_holds_exactly_the_cases():
    assert set(GOLDEN_TRACE) == set(CASES)
    assert all(GOLDEN_TRACE[k] for k in GOLDEN_TRACE)


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_pass_issues_the_recorded_calls(key):
    got, want = recorder.record(CASES[key]), GOLDEN_TRACE[key]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"{key}: first difference at call {i}\n  recorded: {w}\n  now:      {g}")
            break
    else:
        if len(got) != len(want):
            print(f"{key}: {len(got)} calls now, {len(want)} recorded; the first {min(len(got), len(want))} agree")
    assert got == want


def test_every_gemm_is_looked_up_on_the_module_when_it_is_called():
    """The stubs were installed after the package was imported and a model was built: a call that reached them was looked up at call time."""
    assert any(line.startswith("gemm(") for line in recorder.record(CASES["frozen.tiny.image.nograd"]))
    assert any(line.startswith("gemm(") for line in recorder.record(CASES["tail1.tiny.text"]))


def stubbed(fn):
    """fn() with the recorder's stubs in place of the kernels."""
    return recorder.record(lambda device, on_model: fn())


def test_a_taped_pass_inside_low_latency_is_refused():
    from proto_clip_amd import ops

    def run():
        model = tower_pass_cases.make_model(TINY, 7, "cpu")
        model.unfreeze(visual_blocks=1, text_blocks=1)
        with ops.low_latency():
            with pytest.raises(PclipError, match=r"encode_image \(visual tower, blocks 1\.\.1 \+ heads trainable\): a differentiable pass inside "
                                                 r"ops\.low_latency\(\) is not supported"):
                model.encode_image(tower_pass_cases.make_images(TINY, "cpu"))
            with pytest.raises(PclipError, match=r"encode_text \(text tower, blocks 1\.\.1 \+ heads trainable\): a differentiable pass inside "
                                                 r"ops\.low_latency\(\) is not supported"):
                model.encode_text(tower_pass_cases.make_tokens(TINY, "cpu"))
    stubbed(run)


def test_a_taped_pass_beyond_the_attention_backward_envelope_is_refused():
    from proto_clip_amd import autograd as pag

    def run():
        kw = dict(TINY, image_resolution=8 * 17)                                 # 17 x 17 patches + 1 = 290 tokens
        model = tower_pass_cases.make_model(kw, 7, "cpu")
        images = torch.zeros(1, 3, kw["image_resolution"], kw["image_resolution"])
        assert model.encode_image(images).shape == (1, kw["embed_dim"])          # frozen: any length
        model.unfreeze(visual_blocks=1)
        with pytest.raises(PclipError, match=rf"sequences of L=290 tokens exceed the attention backward's envelope \(L <= {pag.TOWER_MAX_L}\)"):
            model.encode_image(images)
        for p in model.visual.transformer.parameters():                          # only the heads train: no attention backward, no limit
            p.requires_grad_(False)
        assert model.encode_image(images).requires_grad
    stubbed(run)


def test_a_trainable_prefix_parameter_without_the_opt_in_is_refused():
    def run():
        model = tower_pass_cases.make_model(TINY, 7, "cpu")
        model.visual.class_embedding.requires_grad_(True)
        model.positional_embedding.requires_grad_(True)
        with pytest.raises(PclipError, match=r"visual tower: parameter visual\.class_embedding requires grad but lies in the frozen prefix"):
            model.encode_image(tower_pass_cases.make_images(TINY, "cpu"))
        with pytest.raises(PclipError, match=r"text tower: parameter positional_embedding requires grad but lies in the frozen prefix"):
            model.encode_text(tower_pass_cases.make_tokens(TINY, "cpu"))
        model.visual._stem_opt_in = model._text_stem_opt_in = True               # opted in: the stem goes on the tape
        assert model.visual._tape_plan() == (0, True) and model._text_tape_plan() == (0, True)
        with pytest.raises(PclipError, match=r"visual\.class_embedding"):         # _tape_from keeps refusing (coop / vpt plan with it)
            model.visual._tape_from()
        with pytest.raises(PclipError, match=r"positional_embedding"):
            model._text_tape_from()
    stubbed(run)
