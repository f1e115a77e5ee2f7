"""`import moda_amd.soft_renderer as sr` in place of the reference's `import soft_renderer as sr` (third_party/softras, whose
rasteriser is CUDA only): `sr.SoftRenderer` with the constructor call of nnutils/moda.py:469-471 and `sr.Mesh`, as far as
nnutils/geom_utils.py:675-694 (render_color) touches them -- `renderer.transform.transformer._eye`, `set_texture_mode`,
`render_mesh`.  The drawing is moda_amd.mesh_render (csrc/raster_kernels.hip).

What is served is the configuration MoDA uses: camera_mode 'look_at' without perspective, an eye on the negative z axis,
aggr_func_rgb 'hard', aggr_func_alpha 'prod', dist_func 'euclidean' at sigma_val <= 1e-10 (where the soft silhouette is the
hard cover mask), texture_type 'vertex', fill_back True, no anti-aliasing, ambient light only.  Every other
option raises NotImplementedError naming it: nothing is approximated silently."""
import math

import torch

from . import _lib as L
from . import mesh_render as R


def _refuse(option, value, served):
    raise NotImplementedError(f"moda_amd.soft_renderer: {option}={value!r} is not implemented (served: {served})")


class Mesh:
    """soft_renderer/mesh.py:9-67: vertices (B,V,3) | (V,3), faces (B,F,3) | (F,3), textures (B,V,C) | (V,C) vertex colours."""

    def __init__(self, vertices, faces, textures=None, texture_res=1, texture_type='surface'):
        if texture_type != 'vertex':
            _refuse("texture_type", texture_type, "'vertex'")
        if not (torch.is_tensor(vertices) and torch.is_tensor(faces)):
            raise TypeError("Mesh: vertices and faces must be device tensors")
        self.vertices = vertices[None] if vertices.dim() == 2 else vertices
        self.faces = faces[None] if faces.dim() == 2 else faces
        self.device = self.vertices.device
        self.texture_type = texture_type
        self.batch_size, self.num_vertices = self.vertices.shape[:2]
        self.num_faces = self.faces.shape[1]
        if textures is None:
            textures = torch.ones(self.batch_size, self.num_vertices, 3, dtype=torch.float32, device=self.device)
        self.textures = textures[None] if textures.dim() == 2 else textures
        self.texture_res = 1


class _LookAt:
    def __init__(self, viewing_angle, viewing_scale, eye):
        self.perspective = False
        self.viewing_angle = viewing_angle
        self.viewing_scale = viewing_scale
        self._eye = eye
        if self._eye is None:                                                 # transform.py:38-39
            self._eye = [0, 0, -(1. / math.tan(math.radians(self.viewing_angle)) + 1)]


class _Transform:
    def __init__(self, transformer):
        self.camera_mode = 'look_at'
        self.transformer = transformer

    def set_eyes(self, eyes):
        self.transformer._eye = eyes


class _Lighting:
    def __init__(self, light_mode, intensity_ambient, color_ambient, intensity_directionals):
        self.light_mode = light_mode
        self.intensity_ambient = intensity_ambient
        self.color_ambient = color_ambient
        self.intensity_directionals = intensity_directionals


class _Rasterizer:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class SoftRenderer(torch.nn.Module):
    """soft_renderer/renderer.py:47-102 with the reference's argument names and defaults; the defaults that MoDA overrides
    (perspective, aggr_func_rgb, light intensities, camera_mode) are refused like any other unserved value."""

    def __init__(self, image_size=256, background_color=[0, 0, 0], near=1, far=100, anti_aliasing=False, fill_back=True,
                 eps=1e-3, sigma_val=1e-5, dist_func='euclidean', dist_eps=1e-4, gamma_val=1e-4, aggr_func_rgb='softmax',
                 aggr_func_alpha='prod', texture_type='surface', camera_mode='projection', P=None, dist_coeffs=None,
                 orig_size=512, perspective=True, viewing_angle=30, viewing_scale=1.0, eye=None, camera_direction=[0, 0, 1],
                 light_mode='surface', light_intensity_ambient=0.5, light_color_ambient=[1, 1, 1],
                 light_intensity_directionals=0.5, light_color_directionals=[1, 1, 1], light_directions=[0, 1, 0]):
        super().__init__()
        if camera_mode != 'look_at':
            _refuse("camera_mode", camera_mode, "'look_at'")
        if perspective:
            _refuse("perspective", perspective, "False")
        if aggr_func_rgb != 'hard':
            _refuse("aggr_func_rgb", aggr_func_rgb, "'hard'")
        if aggr_func_alpha != 'prod':
            _refuse("aggr_func_alpha", aggr_func_alpha, "'prod'")
        if dist_func != 'euclidean':
            _refuse("dist_func", dist_func, "'euclidean'")
        if not sigma_val <= 1e-10:
            _refuse("sigma_val", sigma_val, "<= 1e-10, where the soft silhouette equals the hard cover mask")
        if anti_aliasing:
            _refuse("anti_aliasing", anti_aliasing, "False")
        if not fill_back:
            _refuse("fill_back", fill_back, "True")
        if light_intensity_directionals != 0:
            _refuse("light_intensity_directionals", light_intensity_directionals, "0")
        if light_mode not in ('vertex', 'surface'):
            raise ValueError('Lighting mode only support surface and vertex')
        self.lighting = _Lighting(light_mode, light_intensity_ambient, light_color_ambient, light_intensity_directionals)
        self.transform = _Transform(_LookAt(viewing_angle, viewing_scale, eye))
        self.rasterizer = _Rasterizer(image_size=image_size, background_color=background_color, near=near, far=far,
                                      anti_aliasing=anti_aliasing, fill_back=fill_back, eps=eps, sigma_val=sigma_val,
                                      dist_func=dist_func, dist_eps=dist_eps, gamma_val=gamma_val, aggr_func_rgb=aggr_func_rgb,
                                      aggr_func_alpha=aggr_func_alpha, texture_type=texture_type)

    def set_sigma(self, sigma):
        if not sigma <= 1e-10:
            _refuse("sigma_val", sigma, "<= 1e-10")
        self.rasterizer.sigma_val = sigma

    def set_gamma(self, gamma):
        self.rasterizer.gamma_val = gamma                                     # only the softmax aggregation reads it

    def set_texture_mode(self, mode):
        assert mode in ['vertex', 'surface'], 'Mode only support surface and vertex'
        if mode != 'vertex':
            _refuse("texture_type", mode, "'vertex'")
        self.lighting.light_mode = mode
        self.rasterizer.texture_type = mode

    def render_mesh(self, mesh, mode=None):
        """-> (B, C + 1, S, S): the C texture channels (3 in the reference; any number here) and alpha."""
        if mode is not None:
            _refuse("mode", mode, "None")
        self.set_texture_mode(mesh.texture_type)
        if self.rasterizer.sigma_val > 1e-10:
            _refuse("sigma_val", self.rasterizer.sigma_val, "<= 1e-10")
        R._forward_only("SoftRenderer.render_mesh", mesh.vertices, mesh.textures)
        verts, tex = L.dev(mesh.vertices.detach()), L.dev(mesh.textures.detach())
        if tex.dim() != 3 or tex.shape[:2] != verts.shape[:2]:
            raise ValueError(f"vertex textures {tuple(tex.shape)} do not match vertices {tuple(verts.shape)}")
        # lighting.py:59-65 with ambient_lighting / directional_lighting: light = ambient * colour + 0 * (...), per vertex
        light = torch.tensor([self.lighting.intensity_ambient * c for c in self.lighting.color_ambient], dtype=torch.float32)
        if not bool((light == 1).all()):
            if tex.shape[-1] != 3:
                raise ValueError("a coloured ambient light needs 3 texture channels")
            tex = tex * light.to(tex.device)
        # transform.py:41-48: look_at(vertices, eye) then orthogonal(scale).  With the eye on the negative z axis look_at's
        # axes are the identity (functional/look_at.py:48-53) and it only subtracts the eye (:59)
        eye = self.transform.transformer._eye
        eye = torch.as_tensor(eye, dtype=torch.float32).reshape(-1)
        if eye.numel() != 3 or float(eye[0]) != 0 or float(eye[1]) != 0 or not float(eye[2]) < 0:
            _refuse("eye", eye.tolist(), "[0, 0, z] with z < 0, for which look_at does not rotate")
        verts = verts - eye.to(verts.device)
        scale = self.transform.transformer.viewing_scale
        if scale != 1.0:                                                      # functional/orthogonal.py:13-16
            verts = torch.stack((verts[..., 0] * scale, verts[..., 1] * scale, verts[..., 2]), -1)
        S = int(self.rasterizer.image_size)
        faces = mesh.faces
        if faces.dim() == 3 and faces.shape[0] == 1 and verts.shape[0] > 1:
            faces = faces[0]                                                  # one face list for every view
        face_idx, bary, _, alpha = R.rasterize(verts, faces, S, near=self.rasterizer.near, far=self.rasterizer.far)
        bg = self.rasterizer.background_color
        if tex.shape[-1] != len(bg):
            if any(b != bg[0] for b in bg):
                raise ValueError(f"{len(bg)} background colours for {tex.shape[-1]} texture channels")
            bg = bg[0]
        img = R.interpolate(tex, faces, face_idx, bary, background=bg)
        return torch.cat([img, alpha[:, None]], 1)

    def forward(self, vertices, faces, textures=None, mode=None, texture_type='surface'):
        return self.render_mesh(Mesh(vertices, faces, textures=textures, texture_type=texture_type), mode)
