"""Float64 references for the ray samplers and the hierarchical resampling stage (moda_amd/rendering.py, csrc/render_kernels.hip:
sample_rays / points / sample_pdf / merge_index / merge_rows / merge_sort), restating the reference's rendering.py:68-89, :105-113
and :582-623 in plain numpy.  Inputs are taken as given (float32 arrays are widened, never re-rounded); nothing here imports the
package.

  sample_z           depths of the S samples of each ray: t = linspace(0, 1, S) (S == 1 gives t = [0], as torch.linspace does),
                     z = near (1 - t) + far t, or 1 / ((1 - t) / near + t / far) with use_disp; stratified jitter with perturb > 0.
  points             rays_o + rays_d z.
  sample_pdf64       the inverse-CDF resampling; also the bin and the divisor each sample actually used.
  merge_with_origin  sort(cat(a, b)) together with where every element came from: the STABLE argsort of the concatenation
                     (on equal keys a before b, then the lower index first)."""
import numpy as np

EPS = 1e-5


def linspace01(n):
    """torch.linspace(0, 1, n) in float64: k / (n - 1); n == 1 -> [0.]."""
    n = int(n)
    if n == 1:
        return np.zeros(1, np.float64)
    return np.arange(n, dtype=np.float64) / float(n - 1)


def sample_z(near, far, S, use_disp=False, perturb=0.0, u=None):
    """near, far (N,) -> z (N, S) float64 (rendering.py:68-83).  u (N, S): the uniforms of the stratified jitter (perturb > 0)."""
    near = np.asarray(near, np.float64).reshape(-1, 1)
    far = np.asarray(far, np.float64).reshape(-1, 1)
    t = linspace01(S)[None, :]
    with np.errstate(all="ignore"):
        if use_disp:
            z = 1.0 / (1.0 / near * (1.0 - t) + 1.0 / far * t)
        else:
            z = near * (1.0 - t) + far * t
    if perturb > 0:
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        upper = np.concatenate([mid, z[:, -1:]], -1)
        lower = np.concatenate([z[:, :1], mid], -1)
        z = lower + (upper - lower) * (float(perturb) * np.asarray(u, np.float64))
    return z


def points(ro, rd, z):
    """rays_o (N, 3), rays_d (N, 3), z (N, S) -> (N, S, 3) float64 (rendering.py:88-89)."""
    ro, rd, z = (np.asarray(x, np.float64) for x in (ro, rd, z))
    return ro[:, None, :] + rd[:, None, :] * z[:, :, None]


def pdf_cdf64(w, eps=EPS):
    """weights (N, nw) -> pdf (N, nw), cdf (N, nw + 1) in float64 (rendering.py:597-600)."""
    w = np.asarray(w, np.float64) + eps
    pdf = w / w.sum(-1, keepdims=True)
    cdf = np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, -1)], -1)
    return pdf, cdf


def sample_pdf64(bins, w, n_imp, u=None, eps=EPS):
    """bins (N, nw + 1), w (N, nw) -> (z, j, D), each (N, n_imp): the samples in float64, the bin `below` every sample fell into
    and the divisor it was interpolated with (cdf[above] - cdf[below], or 1 where that is under eps or the bin is the empty one
    past the end).  u None: the deterministic linspace(0, 1, n_imp).  Written as oracle/moda_oracle.py::sample_pdf writes it."""
    bins = np.asarray(bins, np.float64)
    n_rays, n_s = np.shape(w)
    _, cdf = pdf_cdf64(w, eps)
    if u is None:
        u = np.broadcast_to(linspace01(n_imp), (n_rays, n_imp))
    u = np.ascontiguousarray(u, np.float64)
    inds = np.stack([np.searchsorted(cdf[i], u[i], side="right") for i in range(n_rays)], 0)
    below = np.maximum(inds - 1, 0)
    above = np.minimum(inds, n_s)
    cdf_b = np.take_along_axis(cdf, below, 1)
    cdf_a = np.take_along_axis(cdf, above, 1)
    bin_b = np.take_along_axis(bins, below, 1)
    bin_a = np.take_along_axis(bins, above, 1)
    denom = cdf_a - cdf_b
    denom = np.where(denom < eps, 1.0, denom)
    return bin_b + (u - cdf_b) / denom * (bin_a - bin_b), below, denom


def merge_with_origin(a, b):
    """a (N, La), b (N, Lb) -> (z, src): src = stable argsort of cat(a, b) along the row, z = cat[src] (bit patterns kept)."""
    cat = np.concatenate([a, b], -1)
    src = np.argsort(cat, axis=-1, kind="stable")
    return np.take_along_axis(cat, src, -1), src
