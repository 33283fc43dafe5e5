"""tools/device_code_diff.py on hand-written listings: a pair that differs only in what a refactor may move passes, a pair that drops an MFMA and
crosses an occupancy step fails on exactly those two — a gate that passes silently would be worse than none."""
import importlib.util
import io
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("device_code_diff", os.path.join(REPO, "tools", "device_code_diff.py"))
dcd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dcd)


def _kernel(idx, name, mfma, vgprs, acc="a", extra=0, spill=0):
    body = ["\tv_mfma_f32_16x16x32_f16 %s[0:3], v[0:3], v[4:7], %s[0:3]" % (acc, acc)] * mfma
    body += ["\tglobal_load_dwordx4 v[0:3], v[8:9], off", "\tds_read_b128 v[4:7], v10", "\ts_waitcnt vmcnt(0) lgkmcnt(0)", "\ts_barrier",
             "\tv_exp_f32_e32 v1, v0", "\tv_cvt_f16_f32_e32 v2, v1", "\tglobal_store_dwordx2 v[8:9], v[2:3], off"]
    body += ["\tscratch_load_dword v3, off, off"] * spill + ["\tv_add_f32_e32 v3, v3, v2"] * (200 + extra - spill) + ["\ts_endpgm"]
    text = "%s:\n; %%bb.0:\n%s\n.Lfunc_end%d:\n" % (name, "\n".join(body), idx)
    meta = ("  - .agpr_count:     0\n    .args:\n      - .offset:         0\n        .size:           8\n    .group_segment_fixed_size: 8448\n"
            "    .name:           %s\n    .private_segment_fixed_size: %d\n    .vgpr_count:     %d\n    .vgpr_spill_count: %d\n" % (name, 4 * spill, vgprs, spill))
    return text, meta


def _listing(path, kernels):
    parts = [_kernel(i, *k) for i, k in enumerate(kernels)]
    with open(path, "w") as f:
        f.write("\t.text\n" + "".join(t for t, _ in parts) + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(m for _, m in parts) + "...\n")


def _run(tmp_path, parent, new):
    for side, kernels in (("parent", parent), ("new", new)):
        os.makedirs(tmp_path / side)
        _listing(tmp_path / side / "unit.s", kernels)
    out = io.StringIO()
    return dcd.compare(str(tmp_path / "parent"), str(tmp_path / "new"), out), out.getvalue()


def test_renamed_registers_a_renamed_kernel_and_a_moved_instruction_pass(tmp_path):
    # 148 -> 152 registers stay on the 3-wave step; two more instructions in 208 are within 1 %
    bad, text = _run(tmp_path, [("walk_kernel<1, 4>", 4, 148), ("ce_transpose_kernel<64>", 0, 27)],
                     [("walk_kernel<1, 4>", 4, 152, "v", 2), ("transpose_kernel<64>", 0, 27)])
    assert bad == 0 and "all kernels pass" in text and "FAIL" not in text, text
    assert "transpose_kernel<64>" in text and "same" in text


def test_a_dropped_mfma_and_an_occupancy_step_fail(tmp_path):
    bad, text = _run(tmp_path, [("walk_kernel<1, 4>", 4, 120), ("other_kernel", 2, 128)], [("walk_kernel<1, 4>", 3, 120), ("other_kernel", 2, 136)])
    assert bad == 2, text
    assert "FAIL unit.s walk_kernel<1, 4>: mfma 4 -> 3" in text
    assert "FAIL unit.s other_kernel: waves 4 -> 3" in text


def test_a_kernel_on_one_side_only_fails(tmp_path):
    bad, text = _run(tmp_path, [("walk_kernel<1, 4>", 4, 120)], [("walk_kernel<1, 4>", 4, 120), ("new_kernel", 1, 32)])
    assert bad == 1 and "new_kernel: only in the new build" in text, text


def test_spills_fail_unless_the_kernel_is_the_parents(tmp_path):
    # an untouched kernel keeps the parent's two spills; a kernel that gains them fails, and so does one that keeps them while anything else moves
    spilled = ("old_kernel", 2, 128, "a", 0, 2)
    bad, text = _run(tmp_path, [spilled, ("walk_kernel<1, 4>", 4, 120), ("moved_kernel", 2, 64, "a", 0, 2)],
                     [spilled, ("walk_kernel<1, 4>", 4, 120, "a", 0, 2), ("moved_kernel", 2, 64, "a", 1, 2)])
    assert bad == 2, text
    assert "FAIL unit.s old_kernel" not in text
    assert "FAIL unit.s walk_kernel<1, 4>: scratch 2; private 8; spill 2" in text
    assert "FAIL unit.s moved_kernel: scratch 2; private 8; spill 2" in text
