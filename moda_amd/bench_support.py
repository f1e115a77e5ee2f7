"""The benchmark's workloads, built from the deterministic synthetic generator (`moda_amd/synth.py`): the `models` / `embeddings`
dicts of BASELINE.json's configurations on the GPU, and `TrainHarness` -- one rank's training step at configs[3] size as the
reference's trainer runs it.  `bench.py` and the GPU tests (through tests/gpu_helpers.py) use the SAME objects, so what the tests
check is what the bench times.  Not part of the drop-in surface."""
import types

import numpy as np
import torch

import moda_amd
from . import synth

DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nerf_from_params(p, **kw):
    m = moda_amd.NeRF(**kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return m.to(DEV).eval()


def make_models(seed, B, with_skin=True, with_feat=False, with_vis=False, alpha=10.0, perturb_bones=False, beta=0.1,
                with_dis=False):
    mp = synth.make_models(seed, B=B, with_skin=with_skin, with_feat=with_feat, with_vis=with_vis,
                           perturb_bones=perturb_bones, beta=beta, with_dis=with_dis)
    models = {"coarse": nerf_from_params(mp["coarse"], in_channels_xyz=63, in_channels_dir=27 + 64, init_beta=beta)}
    if B > 0:
        models["bones"] = torch.nn.Parameter(T(mp["bones_rst"]))
        models["bones_rst"] = T(mp["bones_rst"])
        models["skin_aux"] = T(mp["skin_aux"])
        rpc = torch.nn.Embedding(1, 128).to(DEV)
        if with_skin:
            models["nerf_skin"] = nerf_from_params(mp["nerf_skin"], D=5, W=64, in_channels_xyz=63 + 128,
                                                   in_channels_dir=0, out_channels=B, raw_feat=True,
                                                   in_channels_code=128)
            rpc.weight.data = T(mp["rest_pose_code"])
        models["rest_pose_code"] = rpc
    if with_dis:
        models["nerf_dis"] = nerf_from_params(mp["nerf_dis"], D=5, W=128, in_channels_xyz=63 + 128, in_channels_dir=0,
                                              out_channels=3, raw_feat=True, in_channels_code=128)
    if with_feat:
        models["nerf_feat"] = nerf_from_params(mp["nerf_feat"], D=5, W=128, in_channels_xyz=63, in_channels_dir=0,
                                               out_channels=16, raw_feat=True, init_beta=1.0)
    if with_vis:
        models["nerf_vis"] = nerf_from_params(mp["nerf_vis"], D=5, W=64, in_channels_xyz=63, in_channels_dir=0,
                                              out_channels=1, raw_feat=True)
    emb = {"xyz": moda_amd.Embedding(3, 10, alpha=alpha), "dir": moda_amd.Embedding(3, 4, alpha=alpha)}
    return models, emb


def make_opts(**kw):
    o = dict(dist_corresp=False, lbs=False, neudbs=True, symm_shape=False, scale_rgb=1.3, rgb_filter=False,
             use_corresp=False, use_corr=False, use_ot=False, s3im_loss=False)
    o.update(kw)
    return types.SimpleNamespace(**o)


def rays_to_gpu(rays):
    return {k: T(v) for k, v in rays.items()}


# ---- the reference's training step at BASELINE configs[3] size, shared by bench.py --mode train and the GPU tests ------------
TRAIN_TERMS = ("img", "sil", "frnd", "flo", "feat", "proj", "vis", "cyc")
TRAIN_WEIGHTS = dict(img_wt=1.0, sil_wt=0.1, frnd_wt=0.01, flow_wt=1.0, feat_wt=0.01, proj_wt=0.02, vis_wt=1.0, cyc_wt=0.05)
# what the no-grad coarse pre-pass of a hierarchical (use_fine) training step runs in, per training precision: the inference
# kernels of the same accuracy class (bf16 training: the bf16 throughput kernels; the fp32-grade modes: split-bf16 / exact fp32)
PREPASS_PRECISION = {"bf16": "bf16", "bf16x3": "bf16x3", "bf16x6": "bf16x3", "fp32": "fp32"}


def make_root_rts(n_frames, data_offset, num_freqs=6, t_embed_dim=128):
    """The reference's default root-pose module (moda.py:376-379) over `n_frames` frames with weights from synth; the head's biases
    are zero, as RTHead's constructor leaves them (nerf.py:319-322)."""
    from moda_amd.feeders import RTExpMLP
    m = RTExpMLP(n_frames, num_freqs, t_embed_dim, np.asarray(data_offset))
    w, b = synth.linear_init(0, "nerf_root_rts.root_code", t_embed_dim, m.root_code.basis_mlp.in_features)
    m.root_code.basis_mlp.load_state_dict({"weight": torch.from_numpy(w), "bias": torch.from_numpy(b)})
    p = synth.nerf_params(0, "nerf_root_rts.mlp_rt", D=8, W=256, in_channels_xyz=t_embed_dim, in_channels_dir=0, out_channels=6)
    m.mlp_rt.load_state_dict({k: torch.from_numpy(v if not k.endswith(".bias") else np.zeros_like(v)) for k, v in p.items()})
    return m


class TrainHarness:
    """One rank's training step as the reference's trainer runs it (nnutils/train_utils.py:950-969): forward + backward of
    the total loss assembled as nnutils/moda.py:540-640 does (default weights), DDP-style gradient all-reduce for world > 1,
    AdamW(betas (0.9, 0.999), weight_decay 1e-4, train_utils.py:227-250).  The learning rate is what OneCycleLR(max_lr 5e-4,
    div_factor 25, train_utils.py:260-288) applies at the start of training: 5e-4 / 25 = 2e-5 (`lr`).

    Everything about a step is a deterministic function of (seed, step index): the rays are fixed, the two random tensors a
    step draws (depth jitter, visibility-loss negatives) come from this object's own generator, also under graph replay.
    `terms` (device, 8 floats) holds the weighted loss terms of the last step in TRAIN_TERMS order; `loss_buf` = [loss * N, N]."""

    def __init__(self, N=2048, S=128, B=25, precision="bf16", rank=0, world=1, dist=None, lr=2e-5, device=None, seed=1000,
                 rays_per_frame=4, fused_adamw=True, bucket=True, use_fine=False, with_unc=False, strong=False, clip_grad=False,
                 clip_scale=10.0, default_losses=False, bone_loc=False, root_pose=False, device_optimizer=False, total_steps=None,
                 num_epochs=None, nf_reset=False):
        """use_fine / with_unc: the reference's LAST training stage (scripts/template.sh:59: --fine_steps 0 --use_unc): S/2 coarse
        depths rendered without gradients (rendering.py:91-107, here on the fused inference kernels in `PREPASS_PRECISION[precision]`),
        S/2 importance samples merged in, and the uncertainty network nerf_unc (8x256, moda.py:457-464) trained on
        | sil * img_loss - unc_pred |^2 (moda.py:707-720) -- BASELINE configs[4] as a training step.
        clip_grad: the reference's stage between backward and the optimiser step (train_utils.py:966, :1154-1311) on the device
        (moda_amd.train_utils.GradClipper, thresholds GRAD_GROUPS x clip_scale, the flag's default 10), after the gradient
        exchange and mean and before `opt.step()`.  Off by default: the benchmarked step is forward + backward + AdamW.
        default_losses: assemble the loss as the reference's default flags do (moda.py:167-168 loss_flt, rm_novp) through
        moda_amd.loss_utils.forward_loss with a device-resident LossFilter in line mode: ray i belongs to frame
        i // rays_per_frame and to line i % rays_per_frame of it.  root_sm stays off unless root_pose is set (the synthetic scene has no camera table).
        Off by default: the default path and the benchmarked step are unchanged.
        bone_loc (with default_losses): the bone-location term of moda.py:681-698 at the reference's bone_loc_reg = 0.1 inside the
        step -- the Sinkhorn divergence (moda_amd.samples_loss) between this harness's bone centres `bones_rst[:, :3] * 10` and
        1000 points drawn on a fixed synthetic rest mesh (synth.make_rest_mesh) from the preallocated uniforms `bone_u`, which
        draw() refills: replay and eager see the same samples.  The synthetic scene has no rest-pose head, so correct_bones is
        not part of it.  Off by default.
        root_pose (with default_losses): the reference's default root poses (moda.py:83-85: root_opt, root_basis 'expmlp', no
        cameras) inside the step -- an RTExpMLP over this harness's frames, one video [0, n_frames), weights from synth; every step
        calls root_pose.compute_rts and the loss runs with root_sm=True on that table; the module's parameters join the optimiser,
        the gradient bucket and the clipper's names (`nerf_root_rts.*`).  The rays stay the synthetic ones.  Off by default.
        device_optimizer: the reference's optimiser and schedule (train_utils.py:226-290) on the device -- moda_amd.optim.DeviceAdamW
        over named_params(): 22 groups, OneCycleLR peaking at `lr` x the group's factor after 2 of `num_epochs` epochs, over
        `total_steps` steps -- in place of the constant-rate torch AdamW, in eager_step and in every capture form; a replayed graph
        follows the schedule.  `opt` is None then and `dev_opt` the optimiser; every parameter must belong to a group.  Off by
        default: the benchmarked step and every other path are unchanged.
        nf_reset (with root_pose): the near-far reset of forward_default (moda.py:485-491, every step once progress >= nf_reset:
        the recipe's last stage) inside the step, right after compute_rts, in eager mode and in every capture form --
        moda_amd.reset_near_far on `frames`, a FrameState over this harness's frames, all marked seen, with the box of
        synth.make_rest_mesh's bounds for a rest mesh; `near_far` is its (n_frames, 2) table.  The harness's rays stay the
        synthetic ones, so the table is produced in the reference's position and NOT consumed.  Off by default: the harness has
        no `frames` then, and the benchmarked step and every other path are unchanged."""
        from moda_amd import sharding
        global DEV
        if nf_reset and not root_pose:
            raise ValueError("TrainHarness: nf_reset=True recomputes the planes from the root poses of compute_rts (root_pose=True)")
        # strong=True: ONE batch of N rays (the one-rank run's rays) cut into contiguous per-rank ranges (sharding.shard_rays), so
        # that the union of the ranks' rays is the single-rank batch; default: every rank owns its own N rays (weak, DDP's lines)
        n_total = N
        if strong:
            lo, hi = sharding.shard_bounds(n_total, rank, world, align=rays_per_frame)
            N = hi - lo
        self.N, self.S, self.B, self.world, self.dist = N, S, B, world, dist
        self.dev = device or DEV
        self.precision = precision
        self.use_fine, self.with_unc = bool(use_fine), bool(with_unc)
        moda_amd.set_train_precision(precision)
        self.prepass_precision = PREPASS_PRECISION[precision]
        # MoDA's default training configuration (moda.py:60-173): coarse + skin + CSE feature + visibility nets, paired-frame
        # correspondence (dist_corresp), Sinkhorn feature matching (use_ot), all per-ray loss keys present
        prev, DEV = DEV, self.dev
        try:
            self.models, self.emb = make_models(0, B, with_feat=True, with_vis=True)
            sd = seed if strong else sharding.rank_seed(seed, rank)
            n_make = n_total if strong else N
            rays = dict(synth.make_rays(sd, n_make, B, rays_per_frame=rays_per_frame))
            rays.update(synth.make_corresp_rays(sd, n_make, B, rays_per_frame=rays_per_frame))
            rays.update(synth.make_feat_rays(sd, n_make, rays_per_frame=rays_per_frame))
            if self.with_unc:
                rays.update(synth.make_unc_rays(sd, n_make, rays_per_frame))
            if strong:
                rays = sharding.shard_rays({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rays.items()}, rank, world)
                rays = {k: v.numpy() for k, v in rays.items()}
            rays = rays_to_gpu(rays)
            if self.with_unc:
                unc = moda_amd.NeRFUnc(in_channels_xyz=63, D=8, W=256, out_channels=1, in_channels_dir=32, raw_feat=True, init_beta=1.)
                unc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_params(
                    0, "nerf_unc", D=8, W=256, in_channels_xyz=63, in_channels_dir=32, out_channels=1, init_beta=1.).items()})
                self.models["nerf_unc"] = unc.to(self.dev)
        finally:
            DEV = prev
        for m in self.models.values():
            if isinstance(m, torch.nn.Module):
                m.train()
        self.models["bones_rst"] = torch.nn.Parameter(self.models["bones_rst"].clone())
        self.models["skin_aux"] = torch.nn.Parameter(self.models["skin_aux"].clone())
        for k in ("bone_rts", "bone_rts_target", "bone_rts_dentrg", "time_embedded", "env_code", "rays_o", "rays_d", "rtk_vec",
                  "rtk_vec_target", "rtk_vec_dentrg"):
            rays[k].requires_grad_(True)
        self.rays = rays
        self.params = [p for m in self.models.values() if isinstance(m, torch.nn.Module) for p in m.parameters()]
        self.params += [self.models["bones_rst"], self.models["skin_aux"]]
        self.root_pose, self.root_rts, self.aux_out = bool(root_pose), None, {}
        if self.root_pose:
            if not default_losses:
                raise ValueError("TrainHarness: root_pose=True feeds the root-smoothness term of the default loss assembly (default_losses=True)")
            self.n_frames = (N + rays_per_frame - 1) // rays_per_frame
            self.data_offset = (0, self.n_frames)
            self.root_rts = make_root_rts(self.n_frames, self.data_offset).to(self.dev).train()
            self.params += list(self.root_rts.parameters())
        self.frames = self.near_far = None
        if nf_reset:
            from moda_amd.frame_state import FrameState
            from moda_amd.mesh import TriMesh
            v, f = synth.make_rest_mesh()
            self.near_far = torch.zeros((self.n_frames, 2), device=self.dev)
            self.frames = self.latest_vars = FrameState(self.n_frames, self.dev, self.near_far)
            self.frames.mesh_rest = TriMesh(torch.from_numpy(v).to(self.dev), torch.from_numpy(f).to(self.dev))
            self.frames.idk.fill_(1.0)
            self.frames.rtk[:, 3] = torch.tensor([1.0, 1.0, 0.0, 0.0], device=self.dev)
            self.frames.box()                                           # the 8 corners go up here, not inside a step
        self.opts = make_opts(dist_corresp=True, use_corresp=True, use_ot=True)
        self.bound = np.asarray([0.2, 0.2, 0.2], np.float32)
        self.loss_buf = torch.zeros(2, device=self.dev)
        self.terms = torch.zeros(len(TRAIN_TERMS), device=self.dev)
        kw = dict(lr=lr, betas=(0.9, 0.999), weight_decay=1e-4, capturable=True)
        self.opt = self.dev_opt = None
        if device_optimizer:
            from moda_amd.optim import DeviceAdamW
            if total_steps is None or num_epochs is None:
                raise ValueError("TrainHarness: device_optimizer=True needs the schedule's total_steps and num_epochs")
            self.dev_opt = DeviceAdamW(self.named_params(), lr, total_steps, 2. / num_epochs, root_basis="expmlp")
            if self.dev_opt.skipped:
                raise ValueError(f"TrainHarness: parameters without an optimiser group: {self.dev_opt.skipped}")
        elif fused_adamw:     # one fused kernel per step (the foreach form issues ~150 one-element divisions for its bias corrections)
            try:
                self.opt = torch.optim.AdamW(self.params, fused=True, **kw)
            except (RuntimeError, TypeError, ValueError):
                self.opt = None
        if self.opt is None and self.dev_opt is None:
            self.opt = torch.optim.AdamW(self.params, **kw)
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(seed * 7919 + rank)
        self.vis_neg = torch.empty((1, N * S, 3), device=self.dev)      # negatives of the visibility loss (loss_utils.py:137)
        S_c = S // 2 if self.use_fine else S                            # coarse depths of a hierarchical step (rendering.py:50)
        self.jitter = torch.empty((N, S_c), device=self.dev)            # depth jitter (rendering.py:82)
        self.pdf_u = torch.empty((N, S_c), device=self.dev) if self.use_fine else None    # resampling uniforms (:607)
        self.noise_pre = torch.zeros((N, S_c), device=self.dev) if self.use_fine else None
        self.feat_noise = torch.empty((1, 8000, 3), device=self.dev)    # lattice jitter of feat_match (loss_utils.py:306)
        self.noise_raw = torch.zeros((N, S), device=self.dev)           # density noise (rendering.py:193): noise_std is 0
        self.graph = self.graph_tail = None
        self.graph_form = "eager"
        self.steps_done = 0
        # bucket: after the first step has shown which network parameters receive a gradient (the heads a network does not
        # evaluate get none, and AdamW must keep skipping them), those parameters' gradients become views of ONE flat buffer
        # that the backward kernels add into directly (moda_amd.GradBucket)
        self.want_bucket = bucket
        self.bucket = None
        self.clip_grad, self.clip_scale = bool(clip_grad), float(clip_scale)
        self.clipper = None
        self.default_losses = bool(default_losses)
        self.loss_filter = None
        if self.default_losses:
            from moda_amd.loss_utils import LossFilter
            n_frames = (N + rays_per_frame - 1) // rays_per_frame
            self.loss_filter = LossFilter(n_frames, 512, lineload=True, device=self.dev)
            idx = torch.arange(N, device=self.dev)
            self.frameid = (idx // rays_per_frame).to(torch.int32)
            self.errid = self.frameid * 512 + (idx % rays_per_frame).to(torch.int32)
            w = TRAIN_WEIGHTS
            self.loss_opts = dict(loss_flt=True, rm_novp=True, root_sm=self.root_pose, bone_loc_reg=0.1 if bone_loc else 0.0, lineload=True,
                                  use_unc=self.with_unc,
                                  img_wt=w["img_wt"], sil_wt=w["sil_wt"], frnd_wt=w["frnd_wt"], flow_wt=w["flow_wt"],
                                  feat_wt=w["feat_wt"], proj_wt=w["proj_wt"], cyc_wt=w["cyc_wt"])

        self.bone_loc = bool(bone_loc)
        if self.bone_loc:
            if not self.default_losses:
                raise ValueError("TrainHarness: bone_loc=True is a term of the default loss assembly (default_losses=True)")
            from moda_amd.mesh import TriMesh
            from moda_amd.samples_loss import SamplesLoss
            v, f = synth.make_rest_mesh()
            self.mesh_rest = TriMesh(torch.from_numpy(v).to(self.dev), torch.from_numpy(f).to(self.dev))
            self.bone_u = torch.empty((1000, 3), device=self.dev)       # uniforms of sample_points_from_meshes
            self.samples_loss = SamplesLoss("sinkhorn", p=2, blur=.05)
            self.bone_loc_value = None                                   # the unweighted term of the last step

    def named_params(self):
        """`self.params` under the names the reference's model gives them (what clip_grad groups by): the networks by their
        attribute names (nerf_coarse, nerf_skin, ...), the rest bones as `bones`."""
        ref = {"coarse": "nerf_coarse"}
        out = [(f"{ref.get(k, k)}.{n}", p) for k, m in self.models.items() if isinstance(m, torch.nn.Module)
               for n, p in m.named_parameters()]
        out = out + [("bones", self.models["bones_rst"]), ("skin_aux", self.models["skin_aux"])]
        if self.root_rts is not None:
            out += [("nerf_root_rts." + n, p) for n, p in self.root_rts.named_parameters()]
        return out

    def _clip(self):
        """The clipping stage, if enabled: three launches, nothing read back (eager and captured alike)."""
        if not self.clip_grad:
            return
        if self.clipper is None:
            from moda_amd.train_utils import GradClipper
            self.clipper = GradClipper(self.named_params(), self.clip_scale)
        self.clipper()

    def _opt_step(self):
        """The optimiser stage: torch's AdamW at a constant rate, or the device optimiser and its schedule (two launches)."""
        if self.dev_opt is not None:
            self.dev_opt.step()
        else:
            self.opt.step()

    @staticmethod
    def _masked_mean(x, m):            # x[m].mean() without the boolean gather (no host sync, graph-capturable)
        m = m.to(x.dtype).expand_as(x)
        return (x * m).sum() / m.sum()

    def draw(self):
        """The step's random tensors, outside any graph (a captured generator needs registration; this does not)."""
        self.vis_neg.uniform_(generator=self.gen)
        self.jitter.uniform_(generator=self.gen)
        self.feat_noise.normal_(generator=self.gen)
        if self.pdf_u is not None:
            self.pdf_u.uniform_(generator=self.gen)
        if self.bone_loc:
            self.bone_u.uniform_(generator=self.gen)

    def fwd_bwd(self):
        from moda_amd.loss_utils import total_loss, unc_loss
        from moda_amd.nerf import precision_scope
        with precision_scope(self.prepass_precision if self.use_fine else None):
            r = moda_amd.render_rays(self.models, self.emb, self.rays, N_samples=self.S, perturb=1.0, noise_std=0.0, opts=self.opts,
                                     img_size=512, obj_bound=self.bound, use_fine=self.use_fine,
                                     rng={"vis_neg_rand": self.vis_neg, "perturb_rand": self.jitter, "feat_noise": self.feat_noise,
                                          "noise_raw": self.noise_raw, "pdf_u": self.pdf_u, "noise_raw_pre": self.noise_pre})
        # moda.py:540-705 as one launch each way; these weights (not the flags' defaults) keep every term of the synthetic scene
        # within two orders of magnitude of the others, and the loss values comparable across rounds
        if self.default_losses:
            return self._fwd_bwd_default_losses(r)
        loss, terms = total_loss(r, TRAIN_WEIGHTS)
        if self.with_unc:
            loss = loss + unc_loss(r)                                  # moda.py:707-720
        loss.backward()
        self.terms.copy_(torch.stack([terms[k] for k in TRAIN_TERMS]))
        return loss.detach()

    def _fwd_bwd_default_losses(self, r):
        """moda.py:517-768 with loss_flt and rm_novp: the filter's three launches, the assembly's one each way, nothing read back.
        `progress` is 1 (past warmup_steps: the silhouette term is filtered too); the visibility term carries the reference's
        0.01 (moda.py:702), not TRAIN_WEIGHTS' vis_wt.  `terms` keeps TRAIN_TERMS' order; its cycle entry is weighted."""
        from moda_amd.loss_utils import forward_loss
        bone_loc = None
        if self.bone_loc:                                              # moda.py:690-695 (no rest-pose head in the synthetic scene)
            samp = moda_amd.sample_points_from_meshes(self.mesh_rest, u=self.bone_u)
            bone_loc = self.samples_loss(self.models["bones_rst"][:, :3] * 10, samp * 10)
            # detached: a tensor kept WITH its graph would keep the bones' gradient-accumulation node of this call alive, and that
            # node runs on the stream of the call that created it -- inside a later capture, on a stream that is not capturing
            self.bone_loc_value = bone_loc.detach()
        rtk_all = None
        if self.root_pose:                                             # moda.py:667-670 over compute_rts (moda.py:1468-1495)
            from moda_amd.root_pose import compute_rts
            rtk_all = compute_rts(self.root_rts, self.n_frames)
            if self.frames is not None:                                # moda.py:485-491, one launch, nothing read back
                from moda_amd.frame_state import reset_near_far
                reset_near_far(self, rtk_all.detach())
        loss, aux = forward_loss(r, self.loss_opts, loss_filter=self.loss_filter, errid=self.errid, frameid=self.frameid, progress=1.0,
                                 bone_loc=bone_loc, rtk_all=rtk_all, data_offset=self.data_offset if self.root_pose else None)
        loss.backward()
        if self.root_pose:
            self.aux_out = {k: aux[k].detach() for k in ("root_sm_loss", "root_rot_sm", "root_trn_sm")}
        keys = ("img_loss", "sil_loss", "feat_rnd_loss", "flo_loss", "feat_loss", "proj_loss", "visibility_loss", "cyc_loss")
        self.terms.copy_(torch.stack([aux[k] for k in keys]))
        self.terms[7].mul_(TRAIN_WEIGHTS["cyc_wt"])
        return loss.detach()

    def zero_grad(self):
        """Every gradient gone: the bucket by one memset (recorded into a captured graph like any launch), the rest set to None."""
        if self.bucket is None:
            if self.opt is not None:
                self.opt.zero_grad(set_to_none=True)
            else:
                for p in self.params:
                    p.grad = None
            return
        inb = {id(p) for p in self.bucket.params}
        for p in self.params:
            if id(p) not in inb:
                p.grad = None
        self.bucket.attach()
        self.bucket.zero()

    def _make_bucket(self):
        """Every parameter that received a gradient in the first step -- the networks' (written directly by NerfFn's backward) and
        the small ones autograd accumulates (bones_rst, skin_aux, the rest-pose code) -- plus the two loss sums, in ONE flat
        buffer: a step's whole exchange is one all-reduce."""
        nets = [p for p in self.params if p.grad is not None]
        old = [p.grad for p in nets]
        self.bucket = moda_amd.GradBucket(nets, extra=2)
        for p, g in zip(nets, old):                  # this step's gradients move into their views
            p.grad.copy_(g)
        self.bucket.extra.copy_(self.loss_buf)
        self.loss_buf = self.bucket.extra

    def eager_step(self):
        from moda_amd import sharding
        self.draw()
        self.zero_grad()
        loss = self.fwd_bwd()
        if self.want_bucket and self.bucket is None:
            self._make_bucket()                      # this step's gradients have moved into the bucket's views: exchanged below
        self.loss_buf[0] = loss * self.N
        self.loss_buf[1] = float(self.N)
        if self.bucket is not None:
            self.bucket.all_reduce(self.dist, self.world, force=sharding.COLLECTIVES_AT_WORLD_1)   # gradients (mean) + loss sums: ONE ~11 MB collective
            # a parameter outside the bucket that receives a gradient after all (it had none in step 1): exchanged like the rest,
            # never applied un-averaged
            inb = self._in_bucket()
            late = [p for p in self.params if id(p) not in inb and p.grad is not None]
            if late:
                sharding.allreduce_gradients(late, self.dist, self.world)
        else:
            sharding.allreduce_gradients(self.params, self.dist, self.world)
            sharding.allreduce_sums(self.loss_buf, self.dist, self.world)
        self._clip()
        self._opt_step()
        self.steps_done += 1
        return self.loss_buf

    def _in_bucket(self):
        return {id(p) for p in self.bucket.params} if self.bucket is not None else set()

    def capture(self, warm=3):
        """The step as HIP graphs, replayed -- it is launch-latency-bound when issued eagerly (~440 launches for ~6 ms of kernel
        time).  `warm` eager steps run first on a side stream (they count as steps).
        One rank: ONE graph (zero the bucket, forward, backward, AdamW).
        Several ranks: TWO graphs around the step's single collective -- [zero, forward, backward, loss sums] | all-reduce of the
        flat bucket (RCCL, eager: one call) | [mean, AdamW].  The collective stays outside the graphs: its capture works in
        thread-local capture mode only (the process group's watchdog thread polls events, which a GLOBAL-mode capture forbids
        process-wide; tools/rccl_probe.py), and MODA_GRAPH_COLLECTIVE=1 selects that single-graph form."""
        import os
        from moda_amd import sharding
        collective = sharding.live(self.world)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm):
                self.eager_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self.bucket is not None:
            # the captured step exchanges the bucket and nothing else: every gradient the warm-up steps produced must live in it,
            # and every rank must hold the same layout
            inb = self._in_bucket()
            stray = [i for i, p in enumerate(self.params) if id(p) not in inb and p.grad is not None]
            if stray:
                raise RuntimeError(f"TrainHarness.capture: parameters {stray} receive gradients outside the gradient bucket")
            if collective:
                self.bucket.check_same_layout_on_all_ranks(self.dist, self.world)
        self.zero_grad()
        n_f = float(self.N)

        def body():
            if self.bucket is not None:
                self.bucket.zero()                    # the memset is part of the replayed step
            g_loss = self.fwd_bwd()
            self.loss_buf[0] = g_loss * self.N
            self.loss_buf[1:2].fill_(n_f)             # (a fill kernel with a constant: no host scalar inside the capture)

        if not collective:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                body()
                self._clip()
                self._opt_step()
            self.graph, self.graph_tail, self.graph_form = graph, None, "one graph"
            return graph
        if self.bucket is None:
            raise RuntimeError("TrainHarness.capture with several ranks needs the gradient bucket (bucket=True)")
        if os.environ.get("MODA_GRAPH_COLLECTIVE") == "1":
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                body()
                self.bucket.all_reduce(self.dist, self.world, force=True)
                self._clip()
                self._opt_step()
            self.graph, self.graph_tail, self.graph_form = graph, None, "one graph with the all-reduce inside"
            return graph
        head, tail = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(head, capture_error_mode="thread_local"):
            body()
        with torch.cuda.graph(tail, capture_error_mode="thread_local"):
            self.bucket.scale(self.world)
            self._clip()
            self._opt_step()
        self.graph, self.graph_tail, self.graph_form = head, tail, "two graphs around one eager all-reduce"
        # the captures themselves execute nothing: parameters and optimiser state are those after `warm` steps
        return head

    def step(self):
        if self.graph is None:
            return self.eager_step()
        self.draw()
        self.graph.replay()
        if self.graph_tail is not None:
            self.bucket.all_reduce(self.dist, self.world, average=False, force=True)
            self.graph_tail.replay()
        self.steps_done += 1
        return self.loss_buf

    def loss(self):
        return float(self.loss_buf[0] / self.loss_buf[1])

    def invalidate_inference_caches(self):
        for m in self.models.values():
            if hasattr(m, "invalidate_packed"):
                m.invalidate_packed()
