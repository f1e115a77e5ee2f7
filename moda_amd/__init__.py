"""moda_amd -- MI355X (gfx950) implementation of MoDA's per-ray rendering hot path.

Mirrors the reference's call surface (nnutils/rendering.py, nerf.py, dual_quat.py and the skinning
subset of geom_utils.py); all arithmetic runs in libmoda_hip.so (include/moda_hip.h).
"""
from .nerf import Embedding, NeRF, NeRFUnc, set_precision, get_precision  # noqa: F401
from .rendering import render_rays, inference, inference_deform, sample_pdf  # noqa: F401
from .geom_utils import (evaluate_mlp, bone_transform, vec_to_sim3, gauss_mlp_skinning, mlp_skinning,  # noqa: F401
                         skinning, neu_dbs, dqs_blend_skinning)
from .dual_quat import (q_normalize, q_mul, dq_mul, dq_normalize, dq_quaternion_conjugate,  # noqa: F401
                        dq_combined_conjugate, dq_inverse)
from .loss_utils import (visibility_loss, compute_pts_exp, feat_match_loss, feat_match, kp_reproj_loss,  # noqa: F401
                         kp_reproj, eikonal_loss, nerf_gradient, compute_gradients_sdf)
from .feeders import (raycast, sample_xy, chunk_rays, FrameCode, DQ_RTHead, correct_bones, correct_rest_pose,  # noqa: F401
                      update_rays, update_delta_rts, reinit_bones)
from .mesh_queries import warp_bw, warp_fw, query_volume  # noqa: F401
from . import mesh  # noqa: F401
from .mesh import TriMesh, marching_cubes, largest_part, extract_mesh  # noqa: F401
from . import mesh_eval  # noqa: F401
from .mesh_eval import (nearest, chamfer_3DDist, fscore, iterative_closest_point, eval_mesh, ICPSolution,  # noqa: F401
                        SimilarityTransform, iterative_closest_point_device, eval_sequence, SequenceEval)
from . import bones  # noqa: F401
from .bones import kmeans, sample_points_from_meshes, sample_surface, KMeansResult  # noqa: F401
from . import mesh_render  # noqa: F401
from . import soft_renderer  # noqa: F401
from .mesh_render import rasterize, interpolate, render_dp, render_mesh  # noqa: F401
from .geom_utils import obj_to_cam, pinhole_cam, render_color, render_flow, mask_aug  # noqa: F401
from . import checkpoint  # noqa: F401
from . import overflow  # noqa: F401
from .autograd import set_train_precision, get_train_precision, GradBucket  # noqa: F401
from . import train_utils  # noqa: F401
from .train_utils import GradClipper, clip_grad, grad_group, GRAD_GROUPS  # noqa: F401
from . import samples_loss  # noqa: F401
from .samples_loss import SamplesLoss  # noqa: F401
from .loss_utils import bone_loc_loss  # noqa: F401
from .feeders import RTHead, RTExplicit, RTExpMLP, id_rows_sum  # noqa: F401
from .geom_utils import K2mat, K2inv, Kmatinv, mat2K, refine_rt, create_base_se3, prepare_ray_cams  # noqa: F401
from . import root_pose  # noqa: F401
from .root_pose import compute_rts, convert_root_pose  # noqa: F401
from . import optim  # noqa: F401
from .optim import DeviceAdamW, build_optimizer, optimizer_step, group_lr_factors  # noqa: F401
from . import pixel_sampling  # noqa: F401
from .pixel_sampling import sample_pxs, topk_rows, gather_obs, unc_ray_inputs  # noqa: F401
from . import frame_state  # noqa: F401
from .frame_state import (FrameState, save_latest_vars, get_near_far, reset_near_far, near_far_to_bound, reset_nf,  # noqa: F401
                          reset_obj_bound)
from . import cse  # noqa: F401
from .cse import (bbox_dp2rnd, resample_dp, ood_check_cse, feat_argmax, match2coords, match2flo,  # noqa: F401
                  compute_flow_cse)
from . import frame_pairs  # noqa: F401
from .frame_pairs import (mask_bbox, compute_crop_params, remap, warp_flow, crop_frames, flow_process,  # noqa: F401
                          fb_flow_check, prepare_frame_pairs)
from .loss_utils import shape_init_loss, rtk_loss, compute_root_sm_loss, compute_root_sm_2nd_loss  # noqa: F401
from .geom_utils import matrix_to_quaternion  # noqa: F401
from . import warmup  # noqa: F401
from .warmup import forward_warmup_shape, forward_warmup_rootmlp, preset_root_rotations, WarmupHarness  # noqa: F401
from . import pose_cnn  # noqa: F401
from .pose_cnn import Encoder, ResNetConv  # noqa: F401
from .checkpoint import build_pose_cnn  # noqa: F401
from .warmup import extract_cams  # noqa: F401
from . import nvs  # noqa: F401
from .nvs import mask_to_pixels, construct_rays_nvs, render_nvs, crop_short_edge, assemble_frames, NVSFrames  # noqa: F401
from . import animate  # noqa: F401
from .animate import (skin_weights, displaced_vertices, warp_fw_frames, vertex_colors_frames, bone_ellipsoids,  # noqa: F401
                      skin_colors, export_sequence, MeshSequence, write_obj, read_obj)
from . import eval_frames as eval_frames_module  # noqa: F401
from .eval_frames import (nerf_render_eval, render_vid, eval_canvases, flow_to_image, image_grid, to_display,  # noqa: F401
                          video_frames, eval_frames, EvalFrames)
from . import cams  # noqa: F401
from .cams import (save_cams, fill_invalid_rotations, CamInit, align_sim3, Sim3Fit, eval_root, load_root,  # noqa: F401
                   visual_hull_align, align_sfm_sim3, draw_cams, draw_cams_pair, render_root_txt)
from .geom_utils import rtk_invert, rtk_compose, rtk_to_4x4  # noqa: F401
from . import seq_render  # noqa: F401
from .seq_render import render_sequence, SeqRender  # noqa: F401
