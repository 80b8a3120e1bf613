"""Every path of the rasterizer backward, on the device: the public operator (k_render.hip's blend backward,
k_preprocess.hip / gft_appearance.h per Gaussian) against float64 autograd of tests/torch_ref.py, one group of upstream
channels at a time, with dL/dmeans3D held to its SMALLEST path instead of its max-norm (helpers.check_path_case; the
parts of dL/dmeans3D: helpers.float64_case_grads; the scene and its shares: helpers.path_scene, whose conditions
tests/test_grad_paths.py asserts on the CPU, together with the oracle at a tenth of these bounds).

Why: test_gpu_parity.py's check_grads compares whole tensors at GRAD_RTOL = 3e-4 of the max-norm under N(0, 1) upstream
values on all five planes at once.  In its scenes the projected mean is 0.99 of |dL/dmeans3D|_inf, the d_ndc term 0.00024
.. 0.0014, the SH direction terms 0.002 .. 0.007: a direction derivative can be 5 .. 15 % off and those tests pass, the
d_ndc term is seen only where it happens to be more than 3e-4 of the largest row, and nothing says that a clamped
colour channel or amplitude occurs at all (teeth below).

The bound everywhere is the project's GRAD_RTOL; only the yardstick changes (smallest path, SH column, row, sum of the
absolute per-Gaussian terms), and none is taken from the device's output.

Measured on the MI355X (error / yardstick, to be compared with 3e-4; the oracle's fp32 figures are in
tests/test_grad_paths.py and next to these in DESIGN.md section 6, "Every path of the rasterizer backward"):
  dL/dmeans3D against its smallest path, per case: color 8.2e-7, phasor[0:2] 6.1e-6, phasor[2] 2.4e-6, phasor[3:7]
  3.2e-6, depth 6.8e-6, acc 9.5e-7, depth_distortion 1.3e-6, all together 1.8e-5 (1.9e-5 in the deterministic mode; the
  smallest path there, d_ndc, is 0.030 of the max-norm and the error 5.3e-7 of it); the same in both binning modes;
  D1 / D2 / no_vdp / phasors_precomp / colors_precomp: 1.2e-5 at worst (D2, phasor[0:2]);
  SH columns <= 2.1e-6, scales / rotations / opacities / means2D <= 2.9e-6, offsets <= 6.9e-7 of their terms;
  isolated Gaussians: 1.4e-5 of a row's own max at worst (the oracle's fp32: the same 1.4e-5).
  So the device stands 15x inside every bound; no kernel and no oracle code needed a change.

Teeth (device library rebuilt from scratch copies, never committed): (1) dndc_in dropped from the distance chain of
k_preprocess.hip, (2) one degree-3 term of gft_appearance.h's sh_dir_grad scaled by 1.1, (3) the amplitude clamp bit
ignored in k_preprocess.hip.  test_gpu_parity.py::test_forward_backward_vs_oracle[base] passes (2) and catches (1) and (3)
(1.4e-3 of |dL/dmeans3D|_inf, 3.6e-3 of |dL/dsh_p|_inf: 4.6x and 12x its bound); this file fails 7, 11 and 16 of its 29
tests, by 1.0 .. 1.9, 4.9e-3 .. 0.28 and 0.7 .. 1.9 of the yardstick against a bound of 3e-4.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
from test_gpu_parity import GRAD_RTOL, binning_mode

pytestmark = pytest.mark.gpu

VARIANT_CASES = [(v, c) for v in Hh.PATH_VARIANTS for c in Hh.path_variant(v)[2]]


def check(tag, variant, case, got, oracle, rows=False):
    scene, inputs, f, ref = Hh.path_reference(variant, oracle)
    paths = () if rows else Hh.case_paths(case, scene, inputs)
    ratios, bad = Hh.check_path_case(tag, case, ref[case], got, paths, GRAD_RTOL, f=f, D=scene["cfg"]["D"], rows=rows)
    print("\n[device] %s %s %s: %s" % (tag, variant, case, ", ".join("%s %.2g" % kv for kv in ratios.items())))
    assert not bad, "\n".join(bad)
    return ratios


@pytest.mark.parametrize("variant,case", VARIANT_CASES)
def test_paths(variant, case, oracle, gpu):
    """base: every upstream case at degree 3.  D1 / D2: degrees 1 and 2 of 16 coefficients (the inactive columns are exact
    zeros).  no_vdp: use_view_dependent_phase off (the SH phase columns are exact zeros, the amplitude still carries the
    view direction).  phasors_precomp: no view direction and -- the reference's backward has its whole phasor chain inside
    `if (shs_p)`, backward.cu:527 -- no distance gradient through the phasor either, no gradient to the phasors, exact
    zeros for both offsets.  colors_precomp: dL/dcolors column by column."""
    scene, inputs, f, ref = Hh.path_reference(variant, oracle)
    got = Hh.gpu_case_grads(scene, gpu, case, inputs=inputs)
    if variant == "phasors_precomp":
        assert got.get("phasors_precomp") is None or not got["phasors_precomp"].any()
    check("atomic", variant, case, got, oracle)


def test_isolated_gaussians_row_by_row(oracle, gpu):
    """12 Gaussians that share no pixel (helpers.isolated_scene), row max-norms over three decades: every row of every
    gradient tensor against GRAD_RTOL of its own max -- the faint rows a whole-tensor norm never looks at."""
    scene, inputs, f, ref = Hh.path_reference("isolated", oracle)
    got = Hh.gpu_case_grads(scene, gpu, "all")
    check("atomic", "isolated", "all", got, oracle, rows=True)


@pytest.mark.parametrize("case", ["all", "depth_distortion"])
@pytest.mark.parametrize("mode", [1, 0], ids=["tile_pull", "whole_frame"])
def test_paths_in_both_binning_modes(mode, case, oracle, gpu):
    scene, inputs, f, ref = Hh.path_reference("base", oracle)
    with binning_mode(mode):
        got = Hh.gpu_case_grads(scene, gpu, case)
    check("binning %d" % mode, "base", case, got, oracle)


def test_paths_in_the_deterministic_backward_mode(tmp_path, oracle, gpu):
    """GFT_BWD_DETERMINISTIC=1 is read when the library loads: a child process, as in
    test_gpu_parity.py::test_deterministic_backward_mode, runs the base scene's eight cases and saves their gradients."""
    child, out = tmp_path / "det_paths.py", tmp_path / "det_paths.npz"
    tests = os.path.dirname(os.path.abspath(__file__))
    child.write_text(
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import helpers\n"
        "from gftorf_amd import api\n"
        "api._TILE_HINTS_PER_CAMERA = False\n"
        "scene, inputs, cases = helpers.path_variant('base')\n"
        "res = {}\n"
        "for case in cases:\n"
        "    g = helpers.gpu_case_grads(scene, torch.device('cuda:0'), case)\n"
        "    res.update({case + '|' + k: v for k, v in g.items() if v is not None})\n"
        "np.savez(%r, **res)\n" % (os.path.dirname(tests), tests, str(out)))
    subprocess.check_call([sys.executable, str(child)], env=dict(os.environ, GFT_BWD_DETERMINISTIC="1"), timeout=300)
    det = np.load(out)
    for case in Hh.GPU_PATH_CASES:
        got = {k.split("|")[1]: det[k] for k in det.files if k.startswith(case + "|")}
        assert "means3D" in got and "shs" in got and "phase_offset" in got
        check("deterministic", "base", case, got, oracle)
