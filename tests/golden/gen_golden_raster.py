"""Generate tests/golden/g29_mesh_render.npz by running the reference's own mesh-drawing code on the CPU (development
container only, like gen_golden.py).

Only soft_renderer/cuda/* needs CUDA; renderer.py, rasterizer.py, transform.py, lighting.py, mesh.py and functional/*.py are
plain torch.  The four extension modules (soft_renderer.cuda.soft_rasterize, .voxelization, .load_textures,
.create_texture_image) get stand-ins in sys.modules; only forward_soft_rasterize does anything: it records the face_vertices
and textures that reach it and calls tests/raster_numpy.py.  skimage.io (imported by load_obj / save_obj for files this never
touches) is an empty module when it is not installed.  The reference's device guard (functional/soft_rasterize.py:111) compares a
torch.device with the string "cpu", which is never equal, so it lets CPU tensors through and nothing had to be replaced.

So G29 pins, on reference-executed code, everything AROUND the kernel: obj_to_cam, pinhole_cam, the eye offset of render_color
and its second subtraction in look_at, the y pre-flip, the face-vertex gathering, the lighting, the channel layout, render_flow's
(w-1) grid and masking.  The kernel restatement itself (raster_numpy) is pinned by the analytic tests of test_raster_oracle.py.
NOT pinned here: render_dp (nnutils/moda.py:931-1022).  nnutils/moda.py cannot be imported in this container (torchvision and
pytorch3d are absent and render_dp calls into both: resized_crop, axis_angle_to_matrix), so its camera sampling, crop and
normalisation are restated in moda_amd/mesh_render.py from the source lines and tested against their own stated properties.

    python tests/golden/gen_golden_raster.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _ref_import import import_reference, REF  # noqa: E402
import raster_numpy as rn  # noqa: E402

SEEN = []          # (face_vertices, textures) of every call that reached the stand-in


def _forward(face_vertices, textures, *rest):
    SEEN.append((face_vertices.detach().numpy().copy(), textures.detach().numpy().copy()))
    return rn.forward_soft_rasterize(face_vertices, textures, *rest)


def install_soft_renderer():
    cuda = types.ModuleType("soft_renderer.cuda")
    cuda.__path__ = []
    sys.modules["soft_renderer.cuda"] = cuda
    for name in ("soft_rasterize", "voxelization", "load_textures", "create_texture_image"):
        m = types.ModuleType("soft_renderer.cuda." + name)
        sys.modules[m.__name__] = m
        setattr(cuda, name, m)
    sys.modules["soft_renderer.cuda.soft_rasterize"].forward_soft_rasterize = _forward
    try:
        import skimage.io  # noqa: F401
    except Exception:
        sk, io = types.ModuleType("skimage"), types.ModuleType("skimage.io")
        io.imread = io.imsave = None
        sk.io = io
        sys.modules.update({"skimage": sk, "skimage.io": io})
    sys.path.insert(0, REF + "/third_party/softras")
    import soft_renderer as sr
    sr.cuda = cuda
    return sr


def sphere_views(sub, radius, seeds, shift=(0.0, 0.0, 0.0)):
    v, f = rn.icosphere(sub, radius)
    vs = np.stack([v @ rn.rotation(s).T + np.asarray(shift) for s in seeds]).astype(np.float32)
    return vs, f


def main():
    _, _, geom, _ = import_reference()
    sr = install_soft_renderer()
    S = 64
    # nnutils/moda.py:469-471 verbatim, except the image size (64 keeps the file small)
    renderer = sr.SoftRenderer(image_size=S, sigma_val=1e-12,
                               camera_mode='look_at', perspective=False, aggr_func_rgb='hard',
                               light_mode='vertex', light_intensity_ambient=1., light_intensity_directionals=0.)
    out = {"image_size": np.int64(S), "eye": np.asarray(renderer.transform.transformer._eye, np.float64)}
    rng = np.random.default_rng(29)

    # cameras
    v = rng.uniform(-1, 1, (3, 40, 3)).astype(np.float32)
    Rm = np.stack([rn.rotation(100 + i) for i in range(3)]).astype(np.float32)
    Tm = (rng.uniform(-0.2, 0.2, (3, 3)) + [0, 0, 3]).astype(np.float32)
    K = np.asarray([[2, 2, 0, 0], [1.5, 2.5, 0.1, -0.2], [3, 3, 0.05, 0.05]], np.float32)
    cam = geom.obj_to_cam(torch.as_tensor(v), torch.as_tensor(Rm), torch.as_tensor(Tm))
    out.update(cam_verts=v, cam_R=Rm, cam_T=Tm, cam_K=K, cam_obj_to_cam=cam.numpy(),
               cam_pinhole=geom.pinhole_cam(cam, torch.as_tensor(K)).numpy())

    # render_color: (a) two views of a sphere, (b) two interpenetrating spheres, one partly and one fully off-screen view
    scenes = {}
    va, fa = sphere_views(2, 0.8, (1, 2))
    scenes["a"] = (va, fa, rng.uniform(0.1, 1, (2, va.shape[1], 3)).astype(np.float32))
    # four views, not three: with a batch of exactly 3 the reference's look_at builds its axes with torch.cross WITHOUT a dim
    # (functional/look_at.py:49-50), which then crosses along the batch axis and zeroes x and y -- a quirk of that one batch size
    v1, f1 = sphere_views(2, 0.6, (3, 3, 3, 5), (-0.25, 0.1, 0.0))
    v2, f2 = sphere_views(1, 0.5, (4, 4, 4, 6), (0.3, -0.1, 0.2))
    vb = np.concatenate([v1, v2], 1)
    vb[1, :, 0] += 0.9                                                        # partly off-screen
    vb[2, :, 1] -= 3.0                                                        # fully off-screen
    fb = np.concatenate([f1, f2 + v1.shape[1]])
    scenes["b"] = (vb, fb, rng.uniform(0.1, 1, (4, vb.shape[1], 3)).astype(np.float32))
    for name, (vs, f, col) in scenes.items():
        SEEN.clear()
        faces = torch.as_tensor(f, dtype=torch.int32)[None].repeat(len(vs), 1, 1)
        img = geom.render_color(renderer, torch.as_tensor(vs), faces, torch.as_tensor(col))
        assert len(SEEN) == 1
        out.update({f"{name}_verts": vs, f"{name}_faces": f.astype(np.int32), f"{name}_colors": col,
                    f"{name}_rendered": img.numpy(), f"{name}_face_vertices": SEEN[0][0], f"{name}_face_textures": SEEN[0][1]})

    # render_flow: the sphere of (a) against a slightly rotated and shifted copy of itself
    vn = (va @ rn.rotation(7).T * 0.02 + va * 0.98 + np.asarray([0.03, -0.02, 0.0])).astype(np.float32)
    SEEN.clear()
    faces = torch.as_tensor(fa, dtype=torch.int32)[None].repeat(len(va), 1, 1)
    flow = geom.render_flow(renderer, torch.as_tensor(va), faces, torch.as_tensor(vn))
    out.update(flow_verts=va, flow_faces=fa.astype(np.int32), flow_verts_n=vn, flow_rendered=flow.numpy(),
               flow_face_vertices=SEEN[0][0], flow_face_textures=SEEN[0][1])
    out["cases"] = np.asarray(["a", "b"])
    path = os.path.join(HERE, "g29_mesh_render.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
