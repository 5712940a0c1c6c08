"""Mint tests/golden/trajeval.npz by running the reference's own ``evaluate_ate`` (the unmodified src/tools/eval_ate.py:113-223,
with ``plot=`` set) on the three pose sets of tests/trajeval_reference.py::golden_cases.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trajeval.py REFERENCE_ROOT

eval_ate.py is executed as it stands; the two modules it imports from its package (``src.config``, ``src.common``) are replaced
by empty ones, because ``evaluate_ate`` touches neither.  ``convert_poses`` cannot run here -- ``get_tensor_from_camera`` needs
mathutils -- and the error uses only the translation, so its three lines that mask and scale (:247-253) are restated below.

Recorded per case: the returned dict, ``ax.get_xlim()`` / ``ax.get_ylim()``, the size of the written PNG, and the data and the
display coordinates (``ax.transData.transform`` at the figure's saved 90 dpi) of both plotted trajectories."""
import importlib.util
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import trajeval_reference as R  # noqa: E402


def load_eval_ate(ref):
    pkg = types.ModuleType("src")
    pkg.__path__ = []
    pkg.config = types.ModuleType("src.config")
    common = types.ModuleType("src.common")
    common.get_tensor_from_camera = None
    sys.modules.update({"src": pkg, "src.config": pkg.config, "src.common": common})
    spec = importlib.util.spec_from_file_location("eval_ate", os.path.join(ref, "src", "tools", "eval_ate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def convert(c2w_list, N, scale, mask):
    """convert_poses :241-256 without the quaternion: [tx, ty, tz] per kept frame"""
    poses = []
    for idx in range(0, N + 1):
        if not mask[idx]:
            continue
        c2w_list[idx][:3, 3] /= scale
        poses.append(c2w_list[idx][:3, 3].clone())
    return torch.stack(poses)


def main():
    warnings.simplefilter("ignore")
    eval_ate = load_eval_ate(os.path.abspath(sys.argv[1]))
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    out = {}
    for name, (est, gt, last, scale) in R.golden_cases().items():
        gt_t, est_t = torch.from_numpy(gt.copy()), torch.from_numpy(est.copy())
        mask = torch.ones(last + 1).bool()
        for idx in range(0, last + 1):
            if torch.isinf(gt_t[idx]).any() or torch.isnan(gt_t[idx]).any():
                mask[idx] = 0
        poses_gt, poses_est = convert(gt_t, last, scale, mask).numpy(), convert(est_t, last, scale, mask).numpy()
        N = poses_gt.shape[0]
        first = dict([(i, poses_gt[i]) for i in range(N)])            # evaluate, :231-233
        second = dict([(i, poses_est[i]) for i in range(N)])
        with tempfile.TemporaryDirectory() as tmp:
            png = os.path.join(tmp, "eval_ate_plot.png")
            res = eval_ate.evaluate_ate(first, second, png)
            out[f"{name}/png_size"] = np.array(Image.open(png).size[::-1])
        fig = plt.gcf()
        ax = fig.axes[0]
        fig.set_dpi(90)                                                # what savefig(dpi=90) draws at
        out[f"{name}/xlim"], out[f"{name}/ylim"] = np.array(ax.get_xlim()), np.array(ax.get_ylim())
        for line, what in zip(ax.lines, ("gt", "est")):
            xy = np.asarray(line.get_xydata(), np.float64)
            out[f"{name}/{what}_xy"], out[f"{name}/{what}_px"] = xy, ax.transData.transform(xy)
        plt.close(fig)
        out[f"{name}/est"], out[f"{name}/gt"] = est, gt
        out[f"{name}/last"], out[f"{name}/scale"] = np.array(last), np.array(scale)
        out[f"{name}/pairs"] = np.array(res["compared_pose_pairs"])
        out[f"{name}/stats"] = np.array([res["absolute_translational_error." + k] for k in ("rmse", "mean", "median", "std", "min", "max")])
    np.savez_compressed(os.path.join(HERE, "trajeval.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
