"""nice_slam_amd -- MI355X-native (gfx950, HIP) implementation of the NICE-SLAM volume-rendering hot
path, drop-in behind the reference's Renderer / decoder / get_samples call surface.

    from nice_slam_amd import Renderer, NICE, get_samples, grid_init, load_bound
    from nice_slam_amd import Mesher, marching_cubes
    from nice_slam_amd import recon        # eval_recon.py / cull_mesh.py: calc_3d_metric, calc_2d_metric, render_depth, cull_mesh, ...
    from nice_slam_amd import bound_from_frames, ConvexBound     # Mesher.get_bound_from_frames: TSDF fusion + convex hull
    from nice_slam_amd import KeyframeSelector                   # Mapper.keyframe_selection_overlap
    from nice_slam_amd import imgeval      # Visualizer.vis: image_metrics (PSNR, SSIM, depth L1, residual maps), evaluate_rendering,
                                           # figure_sheet and Visualizer (the 2 x 3 tracking / mapping figure), colorize_depth
    from nice_slam_amd import get_dataset, FramePreparer         # src/utils/datasets.py: the sequence readers, frames prepared on the GPU
    from nice_slam_amd import viewer       # visualizer.py / src/tools/viz.py: Replay, render_mesh, draw_points (headless replay)
    from nice_slam_amd import encode_jpeg, save_jpeg, MjpegWriter    # JPEG files encoded on the GPU, Motion-JPEG video (vis.avi)
    from nice_slam_amd import decode_jpeg, read_jpeg, MjpegReader    # ... and decoded there: Pillow's pixels, bit for bit
    from nice_slam_amd import decode_png, read_png, probe_png        # PNG depth and colour frames decoded on the GPU
    from nice_slam_amd.slam import NICE_SLAM, load_config        # run.py: the run from its config; poses on the device (Trajectory)
    from nice_slam_amd import evaluate_ate, ate_curve            # src/tools/eval_ate.py: alignment, error statistics, eval_ate_plot.png

No CPU / PyTorch fallback exists: every arithmetic entry point goes through libnsr.so.
"""
from .common import aabb_keep, get_camera_from_tensor, get_samples, get_rays, grid_init, load_bound, to_channels_last  # noqa: F401
from .decoders import NICE, MLP, MLP_no_xyz  # noqa: F401
from .renderer import Renderer  # noqa: F401
from .optim import FlatAdam, MaskedGridAdam  # noqa: F401
from .frustum import FrustumSelector  # noqa: F401
from .keyframes import KeyframeSelector  # noqa: F401
from .mapping import backward, get_samples_window, mapping_loss, seed_pixel_draws, tracking_loss  # noqa: F401
from . import graphs  # noqa: F401
from .mesher import Mesher, marching_cubes  # noqa: F401
from . import recon  # noqa: F401
from .recon import align_icp, calc_3d_metric, cull_mesh, nearest, sample_surface  # noqa: F401
from . import bound  # noqa: F401
from .bound import ConvexBound, bound_from_frames, surface_points, tsdf_fuse  # noqa: F401
from . import imgeval  # noqa: F401
from .imgeval import Visualizer, colorize_depth, evaluate_rendering, figure_sheet, image_metrics  # noqa: F401
from . import datasets  # noqa: F401
from .datasets import FramePreparer, get_dataset  # noqa: F401
from . import viewer  # noqa: F401
from . import jpeg  # noqa: F401
from .jpeg import MjpegReader, MjpegWriter, decode_jpeg, encode_jpeg, probe_jpeg, read_jpeg, read_video, save_jpeg  # noqa: F401
from . import png  # noqa: F401
from .png import decode_png, probe_png, read_png  # noqa: F401
from . import poses  # noqa: F401
from .poses import Trajectory, get_tensor_from_camera  # noqa: F401
from . import trajeval  # noqa: F401
from .trajeval import AteResult, ate_curve, evaluate_ate, plot_trajectories, save_plot  # noqa: F401

__all__ = ["Renderer", "NICE", "MLP", "MLP_no_xyz", "get_samples", "get_rays", "grid_init", "load_bound",
           "to_channels_last", "MaskedGridAdam", "FlatAdam", "FrustumSelector", "KeyframeSelector", "aabb_keep", "get_samples_window", "mapping_loss", "tracking_loss", "seed_pixel_draws", "get_camera_from_tensor", "backward",
           "Mesher", "marching_cubes",
           "recon", "nearest", "sample_surface", "align_icp", "calc_3d_metric", "cull_mesh",
           "bound", "bound_from_frames", "ConvexBound", "tsdf_fuse", "surface_points",
           "imgeval", "image_metrics", "evaluate_rendering", "figure_sheet", "colorize_depth", "Visualizer",
           "datasets", "get_dataset", "FramePreparer",
           "viewer",
           "jpeg", "encode_jpeg", "save_jpeg", "MjpegWriter", "decode_jpeg", "probe_jpeg", "read_jpeg", "read_video", "MjpegReader",
           "png", "decode_png", "probe_png", "read_png",
           "poses", "Trajectory", "get_tensor_from_camera",
           "trajeval", "evaluate_ate", "ate_curve", "plot_trajectories", "save_plot", "AteResult"]
