"""The oracle of the optimiser stage (moda_amd/optim.py, csrc/optim_kernels.hip): torch's OneCycleLR restated in Python floats
(float64) and torch's single-tensor AdamW restated in numpy fp32 with a stated operation order.  tests/test_optim_oracle.py holds
both against torch on the CPU; tests/test_gpu_optim.py holds the kernels against them."""
import math

import numpy as np

BETA1, BETA2, EPS, WEIGHT_DECAY = 0.9, 0.999, 1e-8, 1e-4
DIV_FACTOR, FINAL_DIV_FACTOR = 25., 1. / 5


def one_cycle_lr(max_lr, total_steps, pct_start, step, div_factor=DIV_FACTOR, final_div_factor=FINAL_DIV_FACTOR):
    """OneCycleLR.get_lr at last_epoch = step (two phases, anneal_strategy 'linear') in torch's float64 operations.  Past total_steps,
    where torch raises, the value of total_steps is held.  Returns (lr, past): past = step > total_steps."""
    past = step > total_steps
    step_num = min(step, total_steps)
    initial_lr = max_lr / div_factor
    min_lr = initial_lr / final_div_factor
    end0, end1 = float(pct_start * total_steps) - 1, float(total_steps) - 1
    if step_num <= end0:
        pct = (step_num - 0.0) / (end0 - 0.0)
        return (max_lr - initial_lr) * pct + initial_lr, past
    pct = (step_num - end0) / (end1 - end0)
    return (min_lr - max_lr) * pct + max_lr, past


def step_factors(lr, k, beta1=BETA1, beta2=BETA2, weight_decay=WEIGHT_DECAY):
    """The three per-parameter scalars of a step, each computed in float64 and rounded once to fp32 -- torch's single-tensor AdamW
    computes them as Python doubles and hands them to fp32 tensor operations: 1 - lr * wd, lr / (1 - beta1^k), sqrt(1 - beta2^k)."""
    return (np.float32(1 - lr * weight_decay), np.float32(lr / (1 - beta1 ** k)), np.float32(math.sqrt(1 - beta2 ** k)))


def adamw_fp32(p, g, m, v, lr, k, beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=WEIGHT_DECAY):
    """One AdamW step (decoupled weight decay, no amsgrad) on fp32 arrays, in place.  Every operation below is one fp32 operation
    with one rounding, in this order (torch.optim.adam._single_tensor_adam, its non-capturable branch):
        p  = p * f0                        f0 = fp32(1 - lr * wd)                    param.mul_
        m  = m + w1 * (g - m)              w1 = fp32(1 - beta1)                      exp_avg.lerp_ (weight < 0.5)
        v  = v * b2                        b2 = fp32(beta2)                          exp_avg_sq.mul_
        v  = v + (w2 * g) * g              w2 = fp32(1 - beta2)                      .addcmul_(grad, grad, value)
        d  = sqrt(v) / f2 + fp32(eps)      f2 = fp32(sqrt(1 - beta2^k))              (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps)
        p  = p - (f1 * m) / d              f1 = fp32(lr / (1 - beta1^k))             param.addcdiv_(exp_avg, denom, value=-step_size)
    lr is a Python float (float64), k the parameter's own 1-based step count."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    f0, f1, f2 = step_factors(lr, k, beta1, beta2, weight_decay)
    w1, b2, w2, e = np.float32(1 - beta1), np.float32(beta2), np.float32(1 - beta2), np.float32(eps)
    p *= f0
    m += w1 * (g - m)
    v *= b2
    v += (w2 * g) * g
    d = np.sqrt(v) / f2 + e
    p -= (f1 * m) / d


class Oracle:
    """DeviceAdamW's bookkeeping around adamw_fp32: parameters by name, each with its group's schedule, its own step count k
    (a parameter steps only when it has a gradient) and its moments; a global step counter t that the schedule reads."""

    def __init__(self, params, groups, max_lr, total_steps, pct_start):
        self.p = {n: np.array(a, np.float32) for n, a in params.items()}
        self.groups, self.max_lr, self.total_steps, self.pct_start = dict(groups), list(max_lr), total_steps, pct_start
        self.m = {n: np.zeros_like(a) for n, a in self.p.items()}
        self.v = {n: np.zeros_like(a) for n, a in self.p.items()}
        self.k = {n: 0 for n in self.p}
        self.t, self.overrun = 0, 0

    def lrs(self, t):
        return [one_cycle_lr(mx, self.total_steps, self.pct_start, t)[0] for mx in self.max_lr]

    def step(self, grads):
        """grads: name -> fp32 array or None.  Returns (the rates applied, the rates after scheduler.step()), float64 lists."""
        lr = self.lrs(self.t)
        self.overrun += self.t > self.total_steps
        for n, g in grads.items():
            if g is None:
                continue
            self.k[n] += 1
            adamw_fp32(self.p[n], np.asarray(g, np.float32), self.m[n], self.v[n], lr[self.groups[n]], self.k[n])
        nxt = self.lrs(min(self.t, self.total_steps) + 1)
        self.t += 1
        return lr, nxt


# ---- the case tests/test_optim_oracle.py and tests/test_gpu_optim.py share ----------------------------------------------------------
CHUNK = 4096
LEARNING_RATE, TOTAL_STEPS, PCT_START, ROOT_BASIS, N_STEPS = 5e-4, 40, 0.2, "cnn", 14        # the peak is at step 7
# (name, numel, standard deviation of the gradient, flag).  Two tensors share nerf_coarse; nerf_beta_feat and skin_aux are 10x
# groups, nerf_root_rts a root-pose group (0.2x for 'cnn'); most of the 22 groups are empty; `mystery.weight` matches no group.
TENSORS = (
    ("nerf_coarse.xyz_encoding_1.0.weight", 9000, 1.0, None),
    ("nerf_coarse.xyz_encoding_1.0.bias", CHUNK, 1e-2, None),                # exactly one chunk
    ("nerf_coarse.beta", 1, 1e-1, None),
    ("nerf_feat.beta", 5, 1e-3, None),
    ("nerf_root_rts.base_rt.se3", CHUNK + 1, 1e-4, None),
    ("rest_pose_code.weight", CHUNK + 1, 1e-6, "misaligned"),                # parameter and gradient start 4 bytes off 16-byte alignment
    ("skin_aux", 5, 1e-5, "late"),                                           # .grad is None in steps 1 and 2: k restarts at 1 in step 3
    ("bones", CHUNK + 5, 1e-3, "zero5"),                                     # its gradient is all zeros in step 5
    ("mystery.weight", 7, 1.0, None),
)


def make_params(seed=0):
    rng = np.random.default_rng(seed)
    return {n: (0.1 * rng.standard_normal(numel)).astype(np.float32) for n, numel, _, _ in TENSORS}


def make_grads(step, seed=0, late_from=3):
    """The gradients of step 1, 2, ... (name -> fp32 array or None).  late_from: the first step in which the 'late' tensor has a
    gradient (1: always -- a captured graph cannot take a new tensor in)."""
    rng = np.random.default_rng([seed, step])
    out = {}
    for n, numel, std, flag in TENSORS:
        g = (std * rng.standard_normal(numel)).astype(np.float32)
        if flag == "late" and step < late_from:
            g = None
        if flag == "zero5" and step == 5:
            g = np.zeros(numel, np.float32)
        out[n] = g
    return out
