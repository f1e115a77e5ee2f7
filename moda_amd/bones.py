"""What the reference does with the extracted rest mesh besides evaluating it, behind the names it imports:

    kmeans_pytorch.kmeans                      ->  moda_amd.kmeans                       (geom_utils.py:885, reinit_bones)
    pytorch3d.ops.sample_points_from_meshes    ->  moda_amd.sample_points_from_meshes    (moda.py:690, the bone-location loss)

The kernels are moda_amd/csrc/bones_kernels.hip.  k-means keeps its whole state on the device -- centres, assignment, the
iteration counter and the `done` flag -- and the host enqueues Lloyd iterations in batches of 16, reading 8 bytes back per
batch (the package reads one scalar and K `nonzero` results per iteration).  Both results are device tensors.  Sums are float64
through a fixed tree, so a call gives the same bits on every run; an empty cluster is refilled by a stated rule (see `kmeans`)
where the package draws a random point."""
import numpy as np
import torch

from . import _lib as L
from . import abi

MAX_K = abi.CONSTANTS["MODA_KMEANS_MAX_K"]
_BATCH = 16                   # Lloyd iterations enqueued per read-back
_SCAN_TILE = abi.CONSTANTS["MODA_MC_SCAN_TILE"]
_MASK64 = (1 << 64) - 1


def splitmix64(z):
    """The mixing function of the empty-cluster rule, on Python integers mod 2^64."""
    z &= _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def empty_cluster_point(seed, iteration, k, K, N):
    """The index of the point that refills cluster k when it is empty in the iteration after `iteration` finished ones."""
    return splitmix64(seed + 0x9E3779B97F4A7C15 * (iteration * K + k + 1)) % N


class KMeansResult(tuple):
    """(choice_cluster, cluster_centers) -- unpacks as the package's pair -- with .iterations, .shift (the last centre shift,
    float) and .counts (K,) int32, the cluster sizes of the last iteration."""

    def __new__(cls, choice_cluster, cluster_centers, iterations, shift, counts):
        self = super().__new__(cls, (choice_cluster, cluster_centers))
        self.choice_cluster, self.cluster_centers = choice_cluster, cluster_centers
        self.iterations, self.shift, self.counts = iterations, shift, counts
        return self


@torch.no_grad()
def kmeans(X, num_clusters, distance='euclidean', cluster_centers=[], tol=1e-4, tqdm_flag=True, iter_limit=0, device=None,
           seed=None, *, init=None):
    """kmeans_pytorch.kmeans for (N,3) points: -> (choice_cluster (N,) int64, cluster_centers (K,3) fp32), both on the device
    (the package returns CPU tensors), as a KMeansResult that also carries .iterations.

    Lloyd iterations until shift^2 < tol, shift = sum_k |centre_k - previous centre_k|, or `iter_limit` iterations
    (0: no limit); choice_cluster is the assignment against the centres before the last update, as in the package.  The
    nearest centre is exact under d = fma(dz, dz, fma(dy, dy, dx * dx)) in fp32 with the lowest index among equal distances.
    Initial centres: X[init] for `init` (K indices), else X[torch.randperm(N, generator seeded by `seed`)[:K]] (the package
    uses np.random.choice: no parity of the random streams).  An empty cluster k takes the point
    X[empty_cluster_point(seed or 0, iterations finished, k, K, N)] (the package takes a random one).  `tqdm_flag` is accepted
    and ignored."""
    if distance != 'euclidean':
        raise NotImplementedError(f"kmeans: distance={distance!r} is not implemented (only 'euclidean', the reference's choice)")
    if cluster_centers is not None and len(cluster_centers) != 0:
        raise NotImplementedError("kmeans: a non-empty cluster_centers is not implemented; pass init= (K indices into X)")
    if not torch.is_tensor(X):
        raise TypeError(f"kmeans: expected a tensor, got {type(X).__name__}")
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"kmeans: expected (N,3) points, got {tuple(X.shape)}")
    K, N = int(num_clusters), int(X.shape[0])
    if K < 1 or K > MAX_K:
        raise ValueError(f"kmeans: num_clusters = {K} outside 1..{MAX_K}")
    if N < K:
        raise ValueError(f"kmeans: {N} points for {K} clusters")
    if N >= 2 ** 31:
        raise ValueError(f"kmeans: N = {N} exceeds int32 indices")
    tol, iter_limit = float(tol), int(iter_limit)
    if iter_limit < 0 or not tol == tol:
        raise ValueError(f"kmeans: tol = {tol}, iter_limit = {iter_limit}")
    if iter_limit == 0 and tol <= 0:
        raise ValueError("kmeans: tol <= 0 without an iter_limit never stops")
    if not X.is_cuda:
        X = X.to(device if device is not None else "cuda")
    x = L.dev(X.detach())
    dev = x.device
    if init is not None:
        init = torch.as_tensor(init).to(device=dev, dtype=torch.int64).reshape(-1)
        if init.numel() != K:
            raise ValueError(f"kmeans: init holds {init.numel()} indices for {K} clusters")
        bad_init = ((init < 0) | (init >= N)).any()
    else:
        gen = torch.Generator(device=dev)
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(seed))
        init = torch.randperm(N, generator=gen, device=dev)[:K]
        bad_init = torch.zeros((), dtype=torch.bool, device=dev)
    finite, bad_init = (bool(v) for v in torch.stack([torch.isfinite(x).all(), bad_init]).cpu())   # one read-back
    if not finite:
        raise ValueError("kmeans: non-finite coordinate in the input")
    if bad_init:
        raise ValueError(f"kmeans: init index outside [0, {N})")
    centers = x[init].contiguous()
    nblk = int(L.load().moda_kmeans_blocks(N))
    assign = torch.empty(N, dtype=torch.int32, device=dev)
    partials = torch.empty((nblk, K, 4), dtype=torch.float64, device=dev)
    counts = torch.zeros(K, dtype=torch.int32, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    shift = torch.zeros(1, dtype=torch.float64, device=dev)
    rule_seed = (0 if seed is None else int(seed)) & _MASK64
    iterations = 0
    while True:
        steps = _BATCH if iter_limit == 0 else min(_BATCH, iter_limit - iterations)
        L.call("moda_kmeans_steps", L.ptr(x), N, K, L.ptr(centers), L.ptr(assign), L.ptr(partials), L.ptr(counts), L.ptr(state),
               L.ptr(shift), tol, iter_limit, rule_seed, steps, L.stream())
        iterations, done = (int(v) for v in state.cpu())                 # the read-back of this batch
        if done:
            break
    return KMeansResult(assign.long(), centers, iterations, float(shift.cpu()), counts)


def _mesh_tensors(verts, faces, what):
    if hasattr(verts, "vertices_t") and hasattr(verts, "faces_t"):          # a TriMesh
        verts, faces = verts.vertices_t, verts.faces_t
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)):
        raise TypeError(f"{what}: expected a TriMesh or (verts, faces) tensors")
    if verts.requires_grad or faces.requires_grad:
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (the sampler has no backward kernel); "
                                  "pass them detached")
    if verts.dim() != faces.dim() or verts.dim() not in (2, 3) or verts.shape[-1] != 3 or faces.shape[-1] != 3:
        raise ValueError(f"{what}: expected (V,3) and (F,3), or (B,V,3) and (B,F,3); got {tuple(verts.shape)} and {tuple(faces.shape)}")
    batched = verts.dim() == 3
    if not batched:
        verts, faces = verts[None], faces[None]
    if verts.shape[0] != faces.shape[0] or verts.shape[0] < 1:
        raise ValueError(f"{what}: batch sizes {verts.shape[0]} and {faces.shape[0]}")
    if faces.shape[1] == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    if verts.shape[1] == 0:
        raise ValueError(f"{what}: the mesh has no vertices")
    if verts.shape[1] >= 2 ** 31 or 3 * faces.shape[1] >= 2 ** 31:
        raise ValueError(f"{what}: V = {verts.shape[1]} or 3 F = {3 * faces.shape[1]} exceeds int32 indices")
    if not verts.is_cuda:
        verts = verts.to("cuda")
    faces = faces.to(verts.device)
    if faces.dtype != torch.int32:
        if faces.is_floating_point():                                       # moda.py:689 passes torch.Tensor(mesh.faces)
            faces = faces.long()
        if bool(((faces < -2 ** 31) | (faces >= 2 ** 31)).any()):
            raise ValueError(f"{what}: face index outside int32")
    return L.dev(verts.detach()), L.dev(faces, torch.int32), batched


def face_cdf(verts, faces):
    """verts (V,3) fp32, faces (F,3) int32 checked device tensors -> areas (F,) fp32, cdf (F,) float64 (inclusive), n_bad (1,)
    int64: the number of faces with an index outside [0, V).  Nothing is read back."""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    areas = torch.empty(F, dtype=torch.float32, device=dev)
    cdf = torch.empty(F, dtype=torch.float64, device=dev)
    nt = -(-F // _SCAN_TILE)
    ws = torch.empty((2, nt), dtype=torch.float64, device=dev)
    n_bad = torch.empty(1, dtype=torch.int64, device=dev)
    L.call("moda_mesh_face_cdf", L.ptr(verts), L.ptr(faces), V, F, L.ptr(areas), L.ptr(cdf), L.ptr(ws[0]), L.ptr(ws[1]),
           L.ptr(n_bad), L.stream())
    return areas, cdf, n_bad


@torch.no_grad()
def sample_surface(verts, faces, u):
    """One mesh: verts (V,3), faces (F,3), u (S,3) fp32 in [0, 1) -> (points (S,3) fp32, face (S,) int32, areas (F,) fp32,
    cdf (F,) float64).  u[:, 0] picks the face in proportion to its area (the first face whose inclusive CDF exceeds
    u0 * total), (u1, u2) the point in it: s = sqrt(u1), p = (1 - s) a + s (1 - u2) b + s u2 c."""
    verts, faces, batched = _mesh_tensors(verts, faces, "sample_surface")
    if batched:
        raise ValueError("sample_surface takes one mesh")
    return _sample_one(verts[0], faces[0], _uniforms(u, verts.device, 1, None)[0], "sample_surface")


def _uniforms(u, dev, B, S):
    if not torch.is_tensor(u):
        raise TypeError("u: expected a tensor")
    if u.dim() == 2:
        u = u[None].expand(B, *u.shape)
    if u.dim() != 3 or u.shape[0] != B or u.shape[2] != 3 or (S is not None and u.shape[1] != S):
        raise ValueError(f"u: expected ({'S' if S is None else S},3) or ({B},{'S' if S is None else S},3), got {tuple(u.shape)}")
    return L.dev(u.detach().to(dev))


def _sample_one(verts, faces, u, what):
    V, F, S = int(verts.shape[0]), int(faces.shape[0]), int(u.shape[0])
    if 3 * S >= 2 ** 31:
        raise ValueError(f"{what}: {S} samples exceed int32 indices")
    dev = verts.device
    areas, cdf, n_bad = face_cdf(verts, faces)
    if not torch.cuda.is_current_stream_capturing():
        chk = torch.stack([torch.isfinite(verts).all().double(), n_bad[0].double(), cdf[-1],
                           ((u >= 0) & (u < 1)).all().double()]).cpu()          # the one read-back
        if not chk[0]:
            raise ValueError(f"{what}: non-finite vertex coordinate")
        if chk[1]:
            raise ValueError(f"{what}: {int(chk[1])} face(s) index a vertex outside [0, {V})")
        if not chk[2] > 0:
            raise ValueError(f"{what}: the mesh has total area {float(chk[2])}")
        if not chk[3]:
            raise ValueError(f"{what}: u outside [0, 1)")
    # (while a graph is being captured nothing may be read back: the checks above are those of the eager warm-up calls; the
    # kernels themselves skip a face with an index outside [0, V) and clamp the face search, so a replay reads nothing out of bounds)
    points = torch.empty((S, 3), dtype=torch.float32, device=dev)
    face = torch.empty(S, dtype=torch.int32, device=dev)
    L.call("moda_mesh_sample", L.ptr(verts), L.ptr(faces), V, F, L.ptr(areas), L.ptr(cdf), L.ptr(u), S, L.ptr(points), L.ptr(face),
           L.stream())
    return points, face, areas, cdf


@torch.no_grad()
def sample_points_from_meshes(verts, faces=None, num_samples=10000, return_normals=False, *, generator=None, u=None):
    """pytorch3d.ops.sample_points_from_meshes for a TriMesh or (verts, faces) tensors -- where the reference builds a
    `Meshes` (moda.py:687-691) pass the mesh, or its tensors, directly: -> points (S,3), or (B,S,3) for (B,V,3) / (B,F,3) input.
    Faces are drawn in proportion to their area and points uniformly inside them, pytorch3d's published construction (see
    `sample_surface`).  The uniforms are `u` ((S,3) shared by the batch, or (B,S,3)) when given, else torch.rand on the device
    with `generator`; the draw itself is a pure function of them.  While a graph is being captured the mesh / `u` validation
    (one read-back) is skipped: the eager warm-up calls make it; the kernels skip bad faces and clamp the face search."""
    if return_normals:
        raise NotImplementedError("sample_points_from_meshes: return_normals=True is not implemented")
    what = "sample_points_from_meshes"
    verts, faces, batched = _mesh_tensors(verts, faces, what)
    B, dev = int(verts.shape[0]), verts.device
    if u is None:
        S = int(num_samples)
        if S < 0:
            raise ValueError(f"{what}: num_samples = {S}")
        u = torch.rand((B, S, 3), generator=generator, device=dev, dtype=torch.float32)
    else:
        u = _uniforms(u, dev, B, None)
    out = torch.stack([_sample_one(verts[b], faces[b], u[b], what)[0] for b in range(B)])
    return out if batched else out[0]
