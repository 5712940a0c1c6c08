"""TEST INFRASTRUCTURE: the tiny synthetic sequence of tests/perf/ate_study.py (14 frames, 120 x 160) as input of the runner
(nice_slam_amd/slam.py) -- as a Replica-layout folder with a default + scene YAML pair, or held in memory."""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests", "perf")):
    if p not in sys.path:
        sys.path.insert(0, p)

PNG_DEPTH_SCALE = 6553.5


def sequence(device="cpu"):
    import ate_study
    import slam_synthetic as ss
    return ss.SyntheticSequence(ate_study.FRAMES, ate_study.HEIGHT, ate_study.WIDTH, device=device, seed=0)


def run_config(seq, schedule=None, input_folder="", output="", **mapping):
    """(default, scene) config dicts: configs/nice_slam.yaml's keys with the tracker / mapper settings of
    tools/slam_synthetic.DEFAULT_CFG under ``schedule`` (default: ate_study.SCHEDULE), and the scene's own part"""
    import ate_study
    import slam_synthetic as ss
    base = copy.deepcopy(ss.DEFAULT_CFG)
    base["mapping"].update(ate_study.SCHEDULE if schedule is None else schedule)
    default = {
        "coarse": True, "sync_method": "strict", "scale": 1, "verbose": False, "occupancy": True, "low_gpu_mem": True,
        "grid_len": {"coarse": 2.0, "middle": 0.32, "fine": 0.16, "color": 0.16, "bound_divisible": 0.32},
        "pretrained_decoders": {"coarse": "pretrained/coarse.pt", "middle_fine": "pretrained/middle_fine.pt"},
        "meshing": {"level_set": 0, "resolution": 64, "eval_rec": True, "clean_mesh": True, "depth_test": False, "mesh_coarse_level": False,
                    "clean_mesh_bound_scale": 1.02, "get_largest_components": False, "color_mesh_extraction_method": "direct_point_query",
                    "remove_small_geometry_threshold": 0.2},
        "tracking": dict(base["tracking"], device="cuda:0", vis_freq=50, vis_inside_freq=25, seperate_LR=False, no_vis_on_first_frame=True,
                         gt_camera=False),
        "mapping": dict(base["mapping"], device="cuda:0", color_refine=False, fix_fine=True, fix_color=False, no_vis_on_first_frame=True,
                        no_mesh_on_first_frame=True, no_log_on_first_frame=True, vis_freq=50, vis_inside_freq=25, mesh_freq=50,
                        ckpt_freq=500, frustum_feature_selection=True, keyframe_selection_method="overlap",
                        save_selected_keyframes_info=False),
        "rendering": {"N_samples": 32, "N_surface": 16, "N_importance": 0, "lindisp": False, "perturb": 0.0},
        "data": {"dim": 3},
        "model": {"c_dim": 32, "coarse_bound_enlarge": 2, "pos_embedding_method": "fourier"},
    }
    for st in default["mapping"]["stage"].values():            # every learning rate the mapper looks up (configs/nice_slam.yaml:71-95)
        for k in ("decoders_lr", "coarse_lr", "middle_lr", "fine_lr", "color_lr"):
            st.setdefault(k, 0.0)
    default["mapping"].update(mapping)
    room = [[float(lo), float(hi)] for lo, hi in seq.room.tolist()]
    scene = {"dataset": "replica",
             "cam": {"H": seq.H, "W": seq.W, "fx": float(seq.fx), "fy": float(seq.fy), "cx": float(seq.cx), "cy": float(seq.cy),
                     "png_depth_scale": PNG_DEPTH_SCALE, "crop_edge": 0},
             "mapping": {"bound": [[float(a), float(b)] for a, b in seq.bound_cfg], "marching_cubes_bound": room},
             "data": {"input_folder": input_folder, "output": output}}
    return default, scene


def merged_config(seq, **kw):
    from nice_slam_amd.slam import update_recursive
    default, scene = run_config(seq, **kw)
    update_recursive(default, scene)
    return default


def write_folder(seq, folder, **kw):
    """the sequence under ``folder``/seq in the Replica layout (tests/frames_reference.write_sequence) and the YAML pair
    ``folder``/default.yaml, ``folder``/scene.yaml (which inherits from it) -> the scene file's path"""
    import yaml
    import frames_reference as FR
    colors, depths, poses = [], [], []
    for k in range(seq.n):
        color, depth, c2w = seq.frame(k)
        colors.append((color.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).cpu().numpy())
        depths.append(np.clip(np.rint(depth.cpu().numpy().astype(np.float64) * PNG_DEPTH_SCALE), 0, 65535).astype(np.uint16))
        p = c2w.cpu().numpy().astype(np.float64)
        p[:3, 1] *= -1.0                                       # the Replica reader flips the y and z axes back (datasets.py)
        p[:3, 2] *= -1.0
        poses.append(p)
    data = os.path.join(str(folder), "seq")
    FR.write_sequence("replica", data, np.stack(colors), np.stack(depths), np.stack(poses))
    default, scene = run_config(seq, input_folder=data, output=os.path.join(str(folder), "out"), **kw)
    scene = dict(scene, inherit_from=os.path.join(str(folder), "default.yaml"))
    with open(os.path.join(str(folder), "default.yaml"), "w") as fh:
        yaml.safe_dump(default, fh)
    with open(os.path.join(str(folder), "scene.yaml"), "w") as fh:
        yaml.safe_dump(scene, fh)
    return os.path.join(str(folder), "scene.yaml")


class MemorySequence:
    """the frames of a SyntheticSequence held on its device, as a frame reader of the runner"""

    def __init__(self, seq, n=None):
        self.frames = [seq.frame(k) for k in range(seq.n if n is None else n)]
        self.poses = [f[2].detach().cpu().clone() for f in self.frames]

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        color, depth, c2w = self.frames[i]
        return i, color, depth, c2w
