"""Generate tests/golden/schedule.npz from the reference's own learning-rate statements.

Runs ONLY where a checkout of the reference is at hand (its path: the first argument, or $GFTORF_REFERENCE); never on a
GPU machine, and no GPU is needed.  The reference's files never travel; only the settings read and the rates recorded do.

  schedule.npz : ``GaussianModel.update_learning_rate(it, opt)`` (scene/gaussian_model.py:294-313) and
                 ``DeformModel.update_learning_rate(it - opt.warm_up)`` (scene/deform_model.py:42-47) for it = 1..7000 -- both
                 sides of ``optimize_offset_start`` = 4000 and of ``warm_up`` = 2000 -- after the reference's own
                 ``training_setup`` under configs/torf.json: the groups' names, their rates before the first call and after
                 every call (float64), and the settings a restatement needs.  The model's tensors are one-element CPU
                 stand-ins: the rates depend on none of them.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ITERATIONS = 7000
SCENE_EXTENT = 4.5              # cameras_extent of a scene: any positive number; it scales the position rates
SETTINGS = ("position_lr_init", "position_lr_final", "position_lr_delay_mult", "position_lr_max_steps", "feature_phase_lr_init",
            "feature_phase_lr_final", "feature_amp_lr_init", "feature_amp_lr_final", "deform_lr_init", "deform_lr_final", "warm_up",
            "optimize_offset_start", "phase_offset_lr", "dc_offset_lr")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["GFTORF_REFERENCE"]
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(HERE, "..", ".."))              # simple_knn, as the reference imports it
    # imported at module level by what is imported below, used by none of the statements run here
    sys.modules.setdefault("plyfile", types.SimpleNamespace(PlyData=None, PlyElement=None))
    for absent in ("cv2", "imageio", "matplotlib", "matplotlib.pyplot", "tqdm", "scipy", "scipy.spatial", "scipy.spatial.transform"):
        try:
            __import__(absent)
        except ImportError:
            sys.modules[absent] = types.ModuleType(absent)
    # the two modules alone: scene/__init__.py imports the dataset readers and what they need
    scene = types.ModuleType("scene")
    scene.__path__ = [os.path.join(ref, "scene")]
    sys.modules["scene"] = scene
    from arguments import ModelParams, OptimizationParams
    from scene.deform_model import DeformModel
    from scene.gaussian_model import GaussianModel

    parser = argparse.ArgumentParser()
    groups = ModelParams(parser), OptimizationParams(parser)
    args = parser.parse_args([])
    for k, v in json.load(open(os.path.join(ref, "configs", "torf.json"))).items():
        setattr(args, k, v)
    opt = groups[1].extract(args)

    zeros = torch.zeros
    torch.zeros = lambda *a, device=None, **k: zeros(*a, **k)       # training_setup asks for device="cuda"
    g = GaussianModel.__new__(GaussianModel)
    for name in ("_xyz", "_features_dc_color", "_features_rest_color", "_features_dc_phase", "_features_rest_phase", "_features_dc_amp",
                 "_features_rest_amp", "_opacity", "_scaling", "_rotation", "_features_seg_color", "_phase_offset", "_dc_offset"):
        setattr(g, name, torch.nn.Parameter(zeros((1, 1))))
    g.isotropic = False
    g.cameras_extent = g.scene_extent = SCENE_EXTENT
    g.deform_model = DeformModel.__new__(DeformModel)
    g.deform_model.deform = torch.nn.Linear(1, 1)
    g.training_setup(opt)
    torch.zeros = zeros

    names = [p["name"] for p in g.optimizer.param_groups]
    initial = np.array([p["lr"] for p in g.optimizer.param_groups], np.float64)
    deform_initial = np.float64(g.deform_model.optimizer.param_groups[0]["lr"])
    rates = np.empty((ITERATIONS, len(names)), np.float64)
    deform = np.empty((ITERATIONS,), np.float64)
    for it in range(1, ITERATIONS + 1):
        g.update_learning_rate(it, opt)
        g.deform_model.update_learning_rate(it - opt.warm_up)
        rates[it - 1] = [p["lr"] for p in g.optimizer.param_groups]
        deform[it - 1] = g.deform_model.optimizer.param_groups[0]["lr"]
    assert opt.warm_up < ITERATIONS and opt.optimize_offset_start < ITERATIONS
    out = dict(names=np.array(names), initial=initial, rates=rates, deform_initial=deform_initial, deform=deform,
               first_iter=np.int64(1), scene_extent=np.float64(SCENE_EXTENT),
               settings=np.array(SETTINGS), values=np.array([float(getattr(opt, k)) for k in SETTINGS], np.float64))
    np.savez_compressed(os.path.join(HERE, "schedule.npz"), **out)
    print("wrote schedule.npz:", names, rates.shape, os.path.getsize(os.path.join(HERE, "schedule.npz")), "bytes")


if __name__ == "__main__":
    main()
