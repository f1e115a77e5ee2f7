"""What the reference runs before the first forward_default call when a first-stage run starts with `--warmup_shape_ep 5
--warmup_rootmlp` (scripts/template.sh:24), device-resident:

  * forward_warmup_shape   (nnutils/moda.py:795-810)   the coarse SDF pulled towards the ellipsoid / sphere of the DensePose
                           template's bound, loss_utils.shape_init_loss;
  * forward_warmup_rootmlp (moda.py:770-793)           the root MLP trained against the camera table, loss_utils.rtk_loss and the
                           second-order root smoothness;
  * preset_root_rotations  (nnutils/train_utils.py:662-666)  the table's rotations written into RTExpMLP's base quaternions;
  * WarmupHarness          (train_utils.py:845-869 warmup_shape)  the warmup_shape_ep x 200 optimiser steps of the shape stage,
                           eager or as one captured graph replayed after each draw of the uniforms;
  * extract_cams           (train_utils.py:794-807 over eval_cam :393-453)  what warmup_pose(pose_cnn_path=...) is for: every frame's
                           DensePose-CSE feature image through the PoseNet (pose_cnn.Encoder + RTHead, loaded by
                           checkpoint.build_pose_cnn) into the frame table, in chunks.

The reference's methods read their inputs off the model object; so do the two forward_warmup_* functions here (`model` is the
DistributedDataParallel-wrapped or bare module).  TRAINING the pose CNN -- warmup_pose with warmup_pose_ep > 0 and no path,
forward_warmup -- is not implemented (pose_cnn.Encoder refuses training mode).  What the reference's extract_cams does after the
CNN has run -- save_cams, align_sfm_sim3, visual_hull_align, render_root_txt, draw_cams -- is moda_amd/cams.py: hand the tensors
extract_cams returns to cams.save_cams.  process_so3_seq (pydensecrf) is not implemented."""
import numpy as np
import torch

from . import loss_utils
from .feeders import RTExpMLP
from .frame_state import FrameState
from .geom_utils import matrix_to_quaternion
from .optim import DeviceAdamW
from .root_pose import compute_rts
from .train_utils import GradClipper

SHAPE_FACTOR = 0.1          # moda.py:803
BOUND_SCALE = 1.2           # moda.py:807
WARMUP_OPTS = dict(bound_factor=2, init_ellips=False, warmup_shape_ep=0, learning_rate=5e-4, clip_scale=10., root_opt=True)   # moda.py:85-113


def _opt(opts, name):
    if isinstance(opts, dict):
        return opts.get(name, WARMUP_OPTS[name])
    return getattr(opts, name, WARMUP_OPTS[name])


def forward_warmup_shape(model, opts, *, u=None):
    """moda.py:795-810 -> (loss, aux_out) with aux_out['shape_init_loss']: shape_init_loss over model.dp_verts_unit * 0.1 with
    bound_factor = opts.bound_factor * 1.2 and use_ellips = opts.init_ellips, through model.nerf_coarse / model.embedding_xyz.
    u (n,3): this step's uniforms on the device (None: 10 000 points drawn there)."""
    model = getattr(model, "module", model)
    total_loss = loss_utils.shape_init_loss(model.dp_verts_unit * SHAPE_FACTOR, getattr(model, "dp_faces", None), model.nerf_coarse,
                                            model.embedding_xyz, bound_factor=_opt(opts, "bound_factor") * BOUND_SCALE,
                                            use_ellips=_opt(opts, "init_ellips"), u=u)
    return total_loss, {'shape_init_loss': total_loss}


def _rtk_table(latest_vars, device):
    """The camera table as rtk_loss reads it.  A FrameState's table is used where it lies; an array (the reference's
    latest_vars['rtk']) is uploaded, which is not capturable."""
    if isinstance(latest_vars, FrameState):
        return latest_vars.rtk
    rtk = latest_vars['rtk'] if isinstance(latest_vars, dict) else latest_vars
    if torch.is_tensor(rtk):
        return rtk if rtk.is_cuda else rtk.to(device=device, dtype=torch.float32)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("forward_warmup_rootmlp: latest_vars['rtk'] is a host array -- copying it is not capturable, keep the "
                           "table in a FrameState")
    return torch.from_numpy(np.ascontiguousarray(np.asarray(rtk), np.float32)).to(device)


def forward_warmup_rootmlp(model, opts):
    """moda.py:770-793 -> (0.1 * rot_loss + 0.01 * compute_root_sm_2nd_loss, aux_out) with the reference's keys 'rot_loss' and
    'warmup_root_sm_loss' ('trn_loss' removed).  The poses of all model.num_fr frames come from root_pose.compute_rts over
    model.nerf_root_rts -- on the zero table the reference's convert_root_pose starts from when model.use_cam, else on
    create_base_se3 -- and are held against model.latest_vars' rtk table (a FrameState: read where it lies, no host copy)."""
    model = getattr(model, "module", model)
    dev = next(model.nerf_root_rts.parameters()).device
    T = int(model.num_fr)
    aux_out = {}
    rt_raw = torch.zeros((T, 3, 4), device=dev) if getattr(model, "use_cam", False) else None       # moda.py:780, :1430-1433
    rtk = compute_rts(model.nerf_root_rts, T, rt_raw=rt_raw, obj_scale=getattr(model, "obj_scale", 1.0), root_opt=_opt(opts, "root_opt"))
    rtk_gt = _rtk_table(model.latest_vars, dev)
    loss_utils.rtk_loss(rtk, rtk_gt, aux_out)
    root_sm_loss = loss_utils.compute_root_sm_2nd_loss(rtk, model.data_offset)
    total_loss = 0.1 * aux_out['rot_loss'] + 0.01 * root_sm_loss
    aux_out['warmup_root_sm_loss'] = root_sm_loss
    del aux_out['trn_loss']
    return total_loss, aux_out


def preset_root_rotations(nerf_root_rts, rtk):
    """The warmup_rootmlp block of train() (train_utils.py:662-666): base_rt.se3[:, 3:] = matrix_to_quaternion(rtk[:, :3, :3]), in
    place and on the device.  rtk (T, 3 | 4, 4): a device tensor, a FrameState (its rtk table) or a host array (uploaded once).
    Anything but RTExpMLP is refused, as in the reference ("compatible with expmlp root basis only")."""
    if not isinstance(nerf_root_rts, RTExpMLP):
        raise NotImplementedError(f"preset_root_rotations: {type(nerf_root_rts).__name__} -- the rotation preset is compatible with "
                                  "the expmlp root basis (RTExpMLP) only")
    se3 = nerf_root_rts.base_rt.se3
    rtk = _rtk_table(rtk, se3.device)
    if (rtk.dtype != torch.float32 or rtk.dim() != 3 or rtk.shape[1] not in (3, 4) or rtk.shape[2] != 4 or rtk.shape[0] != se3.shape[0]
            or se3.shape[1] != 7):
        raise ValueError(f"rtk: expected fp32 ({se3.shape[0]}, 4, 4) or ({se3.shape[0]}, 3, 4) for a base table of {tuple(se3.shape)}, "
                         f"got {rtk.dtype} {tuple(rtk.shape)}")
    with torch.no_grad():
        se3.data[:, 3:] = matrix_to_quaternion(rtk.detach()[:, :3, :3])
    return nerf_root_rts


def extract_cams(pose_cnn, dp_feats, frameid, dataid, ks_param, kaug, state, *, dp_embed=None, dps=None, unc_filter=False, chunk=50,
                 normalize=True, rt_raw=None):
    """The loop of v2s_trainer.extract_cams / eval_cam (train_utils.py:794-807, 393-453) up to the filled frame table: every
    frame's DensePose-CSE feature image through the PoseNet `pose_cnn` = nn.Sequential(Encoder, RTHead) in chunks of `chunk` frames
    (the reference: 50), the result written into `state` (a FrameState) as save_latest_vars does.

    dp_feats (N,16,H,W) fp32 on the device; frameid (N,) the frames' rows in the tables (video offset included); dataid (N,);
    ks_param (n_videos,4); kaug (N,4).  Per chunk: F.normalize(dp_feats, 2, 1) (moda.py:1399; normalize=False: the features are
    normalised already), with unc_filter ood_check_cse against dp_embed (V,16) and dps (N,H',W'), convert_root_pose(dp_feats=) on
    create_base_se3 (use_cam=False, as warmup_pose sets it), save_latest_vars.  rt_raw (N,3,4): what the table's rt_raw rows
    receive; None: the CNN's poses, which is what the reference's table holds once save_cams has run (train_utils.py:789).

    -> (rtk (N,4,4), is_valid (N,) bool, err_valid (N,) fp32), device tensors; nothing is read back.  The module must be in eval
    mode (checkpoint.build_pose_cnn returns it so).  A frame's result does not depend on `chunk`.  The reference's
    extract_cams ends in save_cams: hand the three returned tensors to cams.save_cams (and cams.align_sfm_sim3 where a video has
    prior cameras; cams.draw_cams draws them).  process_so3_seq (pydensecrf) is not implemented."""
    from types import SimpleNamespace

    from .cse import ood_check_cse
    from .frame_state import save_latest_vars
    from .pose_cnn import normalize_feats
    from .root_pose import convert_root_pose
    if not isinstance(state, FrameState):
        raise TypeError("extract_cams: state must be a moda_amd.FrameState")
    if not torch.is_tensor(dp_feats) or dp_feats.dim() != 4:
        raise ValueError("extract_cams: dp_feats must be a (N, C, H, W) tensor")
    N, chunk = dp_feats.shape[0], int(chunk)
    if chunk < 1 or N < 1:
        raise ValueError(f"extract_cams: {N} frames in chunks of {chunk}")
    if unc_filter and (dp_embed is None or dps is None):
        raise ValueError("extract_cams: unc_filter needs dp_embed (V,16) and dps (N,H,W)")
    kaug = kaug.reshape(-1, 4)
    for t, what in ((frameid, "frameid"), (dataid, "dataid"), (kaug, "kaug"), (rt_raw, "rt_raw"), (dps if unc_filter else None, "dps")):
        if t is not None and t.shape[0] != N:
            raise ValueError(f"extract_cams: {what} holds {t.shape[0]} entries for {N} frames")
    dev = dp_feats.device
    rtk_all = torch.empty((N, 4, 4), device=dev)
    is_valid = torch.ones((N,), device=dev, dtype=torch.bool)
    err_valid = torch.zeros((N,), device=dev)
    with torch.no_grad():
        for i in range(0, N, chunk):
            sl = slice(i, min(i + chunk, N))
            feats = dp_feats[sl]
            if normalize:
                feats = normalize_feats(feats)
            if unc_filter:
                is_valid[sl], err_valid[sl] = ood_check_cse(feats, dp_embed, dps[sl])
            rtk = convert_root_pose(pose_cnn, frameid[sl], dataid[sl], ks_param, dp_feats=feats)
            rtk_all[sl] = rtk
            save_latest_vars(SimpleNamespace(rtk=rtk, kaug=kaug[sl], rt_raw=rtk[:, :3] if rt_raw is None else rt_raw[sl],
                                             frameid=frameid[sl], latest_vars=state))
    return rtk_all, is_valid, err_valid


class WarmupHarness:
    """v2s_trainer.warmup_shape (train_utils.py:845-869): warmup_shape_ep x steps_per_epoch optimiser steps of
    forward_warmup_shape on `nerf_coarse`, with the optimiser and schedule init_training builds for that stage -- AdamW with
    OneCycleLR over warmup_shape_ep * steps_per_epoch steps, pct_start = 2 / warmup_shape_ep -- and clip_grad before each step.

    A step is draw() -- the preallocated uniforms `u` (nsample,3) refilled from this object's own device generator, outside any
    graph -- then zero the gradient bucket, shape_init_loss, backward, GradClipper, DeviceAdamW.  It runs eagerly, or, after
    capture(), as ONE graph replayed after each draw(); both routes issue the same launches on the same data.  The template's
    scaled vertices and their bound are computed once.  Only the parameters the sigma branch uses (xyz_encoding_*, sigma) are
    optimised: the others receive no gradient in this stage, and torch's AdamW skips them too.

    Which bits repeat.  Everything this stage adds is bit-stable from run to run.  The network's own backward is not entirely:
    it forms sigma.bias's gradient -- here exactly sum(dy) -- with float atomics over one workgroup per 32 samples, so the step
    writes the fixed-order sum that the loss' backward leaves (shape_init_loss(dy_sum=)) over that one gradient before clipping.
    Its weight-gradient GEMMs split their reduction over workgroups that add with float atomics once there are 512 samples or
    more (train_kernels.hip, split_k = min(512 / tiles, M / 256)), and the bf16 training precision's backward always does.  So
    in the exact fp32 training precision below 512 samples the eager and the replayed route leave the same bits step after
    step; at the reference's 10 000 samples, or in bf16, two runs of either route agree only to the last bits of those sums.

    step() -> the loss of that step, a 0-dim device tensor (the same buffer every step); loss() reads it back; run(epochs=None)
    does the remaining steps of `epochs` epochs (default: all of warmup_shape_ep).  After run() the caller builds a fresh
    optimiser for the main loop, as the reference's second init_training() does: this object's AdamW state and schedule end with
    the stage."""

    def __init__(self, nerf_coarse, embedding_xyz, dp_verts_unit, opts, *, steps_per_epoch=200, seed=0, nsample=10000):
        self.net, self.embed = nerf_coarse, embedding_xyz
        self.epochs = int(_opt(opts, "warmup_shape_ep"))
        self.steps_per_epoch, self.nsample = int(steps_per_epoch), int(nsample)
        if self.epochs < 1 or self.steps_per_epoch < 1 or self.nsample < 1:
            raise ValueError(f"WarmupHarness: warmup_shape_ep {self.epochs}, steps_per_epoch {steps_per_epoch}, nsample {nsample} "
                             "must all be positive")
        self.bound_factor = _opt(opts, "bound_factor") * BOUND_SCALE
        self.use_ellips = bool(_opt(opts, "init_ellips"))
        verts = loss_utils._warm_tensor(dp_verts_unit, "dp_verts_unit", "(V, 3)", lambda s: len(s) == 2 and s[0] >= 1 and s[1] == 3)
        self.dev = verts.device
        with torch.no_grad():
            self.pts = (verts.detach() * SHAPE_FACTOR).contiguous()
            self.obj_bound = self.pts.abs().amax(0)
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(int(seed))
        self.u = torch.zeros((self.nsample, 3), device=self.dev)
        self.loss_buf = torch.zeros((), device=self.dev)
        self.dy_sum = torch.zeros((1,), device=self.dev)
        from .autograd import GradBucket
        used = [(n, p) for n, p in nerf_coarse.named_parameters() if n.startswith("xyz_encoding_") and "final" not in n or n.startswith("sigma.")]
        self.named = [("nerf_coarse." + n, p) for n, p in used]
        self.bucket = GradBucket([p for _, p in used])
        self.sigma_bias = nerf_coarse.sigma.bias
        self.clipper = GradClipper(self.named, _opt(opts, "clip_scale"))
        self.total_steps = self.epochs * self.steps_per_epoch
        self.opt = DeviceAdamW(self.named, _opt(opts, "learning_rate"), self.total_steps, 2. / self.epochs)
        self.graph = None
        self.steps_done = 0

    def draw(self):
        """This step's uniforms, outside any graph (a captured generator needs registration; this does not)."""
        self.u.uniform_(generator=self.gen)

    def _body(self):
        self.bucket.zero()
        loss = loss_utils.shape_init_loss(self.pts, None, self.net, self.embed, self.bound_factor, self.use_ellips, u=self.u,
                                          obj_bound=self.obj_bound, dy_sum=self.dy_sum)
        loss.backward()
        self.sigma_bias.grad.copy_(self.dy_sum)               # the fixed-order sum over the atomic one (see the class docstring)
        self.loss_buf.copy_(loss.detach())
        self.clipper()
        self.opt.step()

    def eager_step(self):
        self.draw()
        self.bucket.attach()
        self._body()
        self.steps_done += 1
        return self.loss_buf

    def _state(self):
        o = self.opt
        return [p.data for _, p in self.named] + [o.step_count, o.seg_step, o.exp_avg, o.exp_avg_sq, o._lr, o.status, self.loss_buf]

    def capture(self, warm=3, restore=False):
        """The step as one HIP graph.  `warm` eager steps run first on a side stream; they count as steps, unless restore=True
        puts parameters, optimiser state, generator and step count back to where they were, so that every step taken afterwards
        is a replay."""
        saved = ([t.clone() for t in self._state()], self.gen.get_state(), self.steps_done) if restore else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm):
                self.eager_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._body()
        if restore:
            with torch.no_grad():
                for t, v in zip(self._state(), saved[0]):
                    t.copy_(v)
            self.gen.set_state(saved[1])
            self.steps_done = saved[2]
        self.graph = graph
        return graph

    def step(self):
        if self.graph is None:
            return self.eager_step()
        self.draw()
        self.graph.replay()
        self.steps_done += 1
        return self.loss_buf

    def loss(self):
        return float(self.loss_buf)

    def run(self, epochs=None):
        n = (self.epochs if epochs is None else int(epochs)) * self.steps_per_epoch
        if n > self.total_steps:
            raise ValueError(f"WarmupHarness.run: {epochs} epochs exceed the schedule's {self.epochs}")
        while self.steps_done < n:
            self.step()
        return self.loss_buf
