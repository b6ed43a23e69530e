"""ctypes binding of libpmhip.so — the MI355X photon-mapping renderer.

This is a thin host-side mirror of the C-ABI (include/pm_api.h); every
compute call goes to HIP kernels. If the library is missing the import of
`Context` fails loudly: there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

from .abi import (LIGHT_TRI_DTYPE, PM_SCENE_MAT_SPEC, PM_SCENE_MAT_TEX, PM_SCENE_TEXTURES, PM_SCENE_WORLD_SPHERE, TEX_REC_DTYPE, TEX_WRAPS, PHOTON_DTYPE, RECORD_DTYPE, PM_ERR_NO_PHOTONS, PM_FILM_TABLE, PM_FILTER_NONE, Camera,
                  Filter, PMConfig, RenderParams, Stats, f32, fptr, iptr, record_pixels)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libpmhip.so")
_lib = None


class PMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pm error {code}: {msg}")
        self.code = code


class NoPhotonsError(PMError):
    pass


def load_library(path=None):
    """Load libpmhip.so (built by `make -C cuda-raytrace_amd`). Raises if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("PMHIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise ImportError(f"libpmhip.so not found at {p}: build it with `make -C cuda-raytrace_amd` "
                          f"(there is no CPU fallback)")
    lib = ctypes.CDLL(p)
    vp, i64, c_int, c_float, c_double = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double
    P_f, P_i = ctypes.POINTER(c_float), ctypes.POINTER(c_int)
    sig = {
        "pm_default_params": (None, [ctypes.POINTER(RenderParams)]),
        "pm_create": (c_int, [ctypes.POINTER(vp), vp]),
        "pm_destroy": (None, [vp]),
        "pm_last_error": (ctypes.c_char_p, [vp]),
        "pm_version": (ctypes.c_char_p, []),
        "pm_add_material": (c_int, [vp, c_int, P_f, P_i]),
        "pm_add_texture_image": (c_int, [vp, P_f, c_int, c_int, c_int, P_f, P_f, P_i]),
        "pm_add_texture_checker": (c_int, [vp, P_f, c_int, P_f, c_int, P_f, P_i]),
        "pm_add_texture_scale": (c_int, [vp, c_int, P_f, c_int, P_f, P_i]),
        "pm_add_material_textured": (c_int, [vp, c_int, c_int, P_i]),
        "pm_add_material_specular": (c_int, [vp, c_int, P_f, P_f, c_float, P_i]),
        "pm_download_record_albedo": (c_int, [vp, P_f, i64]),
        "pm_upload_record_albedo": (c_int, [vp, P_f, i64]),
        "pm_add_trimesh": (c_int, [vp, P_f, c_int, P_i, c_int, P_f, P_f, c_int, c_int]),
        "pm_add_object_mesh": (c_int, [vp, P_f, c_int, P_i, c_int, P_f, P_f, c_int, c_int, P_i]),
        "pm_add_mesh_instance": (c_int, [vp, c_int, P_f, P_f]),
        "pm_add_sphere": (c_int, [vp, c_float, P_f, P_f, c_int, c_int]),
        "pm_add_disk": (c_int, [vp, P_f, P_f, P_f, P_f, c_float, c_float, c_int, c_int]),
        "pm_add_light_point": (c_int, [vp, P_f, P_f]),
        "pm_add_light_disk": (c_int, [vp, P_f, P_f, P_f, P_f, P_f, c_float, c_int]),
        "pm_add_light_mesh": (c_int, [vp, P_f, c_int, P_i, c_int, c_int, P_f, c_int, P_i]),
        "pm_add_light_distant": (c_int, [vp, P_f, P_f, P_i]),
        "pm_set_pinhole": (c_int, [vp, P_f, P_f, P_f, P_f, c_int, c_int]),
        "pm_set_eye_rays": (c_int, [vp, P_f, i64, P_f, c_int]),
        "pm_set_camera": (c_int, [vp, ctypes.POINTER(Camera)]),
        "pm_film": (c_int, [vp, vp, vp, vp]),
        "pm_camera_rays": (c_int, [vp, i64, i64, P_f, P_f]),
        "pm_camera_rays_pass": (c_int, [vp, c_int, i64, i64, P_f, P_f]),
        "pm_eye_resample": (c_int, [vp, ctypes.POINTER(RenderParams), c_int, vp]),
        "pm_render_resampled": (c_int, [vp, ctypes.POINTER(RenderParams), P_f, ctypes.POINTER(Stats)]),
        "pm_final_gather_pass": (c_int, [vp, ctypes.POINTER(RenderParams), c_int, c_int, vp]),
        "pm_final_gather_resolve": (c_int, [vp, i64, i64, vp, vp]),
        "pm_render_final_gather": (c_int, [vp, ctypes.POINTER(RenderParams), c_int, P_f, ctypes.POINTER(Stats)]),
        "pm_final_gather_rays": (c_int, [vp, ctypes.POINTER(RenderParams), c_int, c_int, i64, i64, P_f]),
        "pm_download_gather_sum": (c_int, [vp, P_f, i64]),
        "pm_set_caustic_map": (c_int, [vp, c_int]),
        "pm_build_caustic_map": (c_int, [vp, vp]),
        "pm_caustic_gather": (c_int, [vp, ctypes.POINTER(RenderParams), c_int, vp]),
        "pm_caustic_map_count": (i64, [vp]),
        "pm_download_caustic_slots": (c_int, [vp, ctypes.POINTER(ctypes.c_uint32), i64]),
        "pm_download_caustic_cell_start": (c_int, [vp, ctypes.POINTER(ctypes.c_uint32), i64]),
        "pm_download_caustic_radiance": (c_int, [vp, P_f, i64]),
        "pm_film_filter_table": (c_int, [ctypes.POINTER(Filter), P_f]),
        "pm_commit": (c_int, [vp]),
        "pm_render": (c_int, [vp, ctypes.POINTER(RenderParams), P_f, ctypes.POINTER(Stats)]),
        "pm_render_simple": (c_int, [vp, ctypes.POINTER(RenderParams), P_f, ctypes.POINTER(Stats)]),
        "pm_simple_pass": (c_int, [vp, ctypes.POINTER(RenderParams), vp, vp]),
        "pm_eye_pass": (c_int, [vp, ctypes.POINTER(RenderParams), vp]),
        "pm_trace_photons": (c_int, [vp, ctypes.POINTER(RenderParams), c_int, i64, i64, i64, vp]),
        "pm_build_photon_map": (c_int, [vp, ctypes.POINTER(RenderParams), i64, vp]),
        "pm_gather": (c_int, [vp, ctypes.POINTER(RenderParams), vp]),
        "pm_gather_partial": (c_int, [vp, ctypes.POINTER(RenderParams), vp, vp]),
        "pm_gather_split": (c_int, [vp, ctypes.POINTER(RenderParams), vp, vp, vp]),
        "pm_ppm_update_split": (c_int, [vp, ctypes.POINTER(RenderParams), vp, vp, i64, i64, vp]),
        "pm_ppm_update_split_radius": (c_int, [vp, ctypes.POINTER(RenderParams), vp, vp, vp]),
        "pm_ppm_update_split_flux": (c_int, [vp, ctypes.POINTER(RenderParams), vp, vp, i64, i64, vp]),
        "pm_ppm_update": (c_int, [vp, ctypes.POINTER(RenderParams), vp, i64, i64, vp]),
        "pm_final": (c_int, [vp, c_double, i64, i64, vp, vp]),
        "pm_num_records": (i64, [vp]),
        "pm_record_pixel": (c_int, [vp, i64, ctypes.POINTER(i64)]),
        "pm_reserve_slots": (c_int, [vp, i64, ctypes.POINTER(vp)]),
        "pm_download_slots": (c_int, [vp, vp, i64]),
        "pm_upload_slots": (c_int, [vp, vp, i64]),
        "pm_download_records": (c_int, [vp, vp, i64]),
        "pm_upload_records": (c_int, [vp, vp, i64]),
        "pm_kdtree_nodes": (i64, [vp]),
        "pm_download_kdtree": (c_int, [vp, vp, i64]),
        "pm_gather_counters": (c_int, [vp, ctypes.POINTER(i64)]),
        "pm_trace_counters": (c_int, [vp, ctypes.POINTER(i64)]),
        "pm_scene_info": (c_int, [vp, ctypes.POINTER(i64)]),
        "pm_scene_section": (c_int, [vp, c_int, vp, i64, ctypes.POINTER(i64)]),
        "pm_map_info": (c_int, [vp, ctypes.POINTER(i64)]),
        "pm_map_grid": (c_int, [vp, ctypes.POINTER(ctypes.c_int32), P_f, ctypes.POINTER(ctypes.c_uint32)]),
        "pm_download_map_cell_start": (c_int, [vp, ctypes.POINTER(ctypes.c_uint32), i64]),
        "pm_download_map_counters": (c_int, [vp, ctypes.POINTER(ctypes.c_uint32), i64]),
        "pm_download_map_photons": (c_int, [vp, P_f, P_f, i64]),
        "pm_download_tile_list": (c_int, [vp, ctypes.POINTER(ctypes.c_uint32), i64, ctypes.POINTER(i64), P_i]),
        "pm_record_view_size": (c_int, [vp, ctypes.POINTER(i64)]),
        "pm_trace_profile": (c_int, [vp, ctypes.POINTER(i64), c_int]),
        "pm_set_counting": (c_int, [vp, c_int]),
        "pm_set_stage_timing": (c_int, [vp, ctypes.c_char_p]),
        "pm_set_record_view": (c_int, [vp, c_int, ctypes.POINTER(i64)]),
        "pm_final_view": (c_int, [vp, c_double, i64, i64, vp, vp]),
        "pm_record_view_list": (c_int, [vp, vp, vp]),
        "pm_synchronize": (c_int, [vp]),
        "pm_last_kernel_ms": (c_int, [vp, ctypes.c_char_p, ctypes.POINTER(c_double)]),
        "pm_halton_permutation": (c_int, [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
        "pm_light_selection_cdf": (c_int, [ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_float), c_int, ctypes.POINTER(ctypes.c_float)]),
        "pm_kdtree_build_host": (i64, [vp, i64, vp]),
        "pm_timing_reset": (c_int, [vp]),
        "pm_gather_range": (c_int, [vp, ctypes.POINTER(RenderParams), i64, i64, vp]),
        "pm_set_slot_buffer": (c_int, [vp, vp, i64]),
        "pm_get_radius2": (c_int, [vp, i64, i64, vp, vp]),
        "pm_set_radius2": (c_int, [vp, vp, i64, i64, vp]),
        "pm_timing_total": (c_int, [vp, ctypes.c_char_p, ctypes.POINTER(i64), ctypes.POINTER(c_double)]),
        "pm_reset_records": (c_int, [vp, ctypes.POINTER(RenderParams), vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if path is None:
        _lib = lib
    return lib


def halton_permutation(seed):
    lib = load_library()
    out = (ctypes.c_uint32 * 28)()
    lib.pm_halton_permutation(seed, out)
    return np.frombuffer(out, dtype=np.uint32).copy()


def light_selection_cdf(types, le_rgb, areas):
    """The light selection table of PM_ALL_LIGHTS (pm_light_selection_cdf; host
    only, no device): float32 cdf per light. Raises ValueError where the call
    returns PM_ERR_INVALID (no lights, unknown type, total weight 0 / not finite)."""
    lib = load_library()
    types = np.ascontiguousarray(np.asarray(types, dtype=np.int32))
    n = int(types.size)
    rgb, ar = f32(le_rgb, 3 * n), f32(areas, n)
    out = np.zeros(max(n, 1), dtype=np.float32)
    rc = lib.pm_light_selection_cdf(iptr(types), fptr(rgb), fptr(ar), n, fptr(out))
    if rc != 0:
        raise ValueError(f"pm_light_selection_cdf failed ({rc}): {lib.pm_last_error(None).decode()}")
    return out[:n]


def film_filter_table(filt, **kw):
    """The film's 16 x 16 weight table (pm_film_filter_table; host only): filt is a Filter or
    the arguments of Filter.make. Raises ValueError where the call returns PM_ERR_INVALID."""
    lib = load_library()
    f = Filter.make(filt, **kw)
    out = np.zeros((PM_FILM_TABLE, PM_FILM_TABLE), dtype=np.float32)
    rc = lib.pm_film_filter_table(ctypes.byref(f), fptr(out))
    if rc != 0:
        raise ValueError(f"pm_film_filter_table failed ({rc}): {lib.pm_last_error(None).decode()}")
    return out


def kdtree_build_host(slots):
    """Canonical pbrt-v2 kd-tree over the valid slots (host, reference layout)."""
    lib = load_library()
    slots = np.ascontiguousarray(slots, dtype=PHOTON_DTYPE)
    nodes = np.zeros(len(slots), dtype=PHOTON_DTYPE)
    n = lib.pm_kdtree_build_host(slots.ctypes.data, len(slots), nodes.ctypes.data)
    return nodes[:n]


class Context:
    """One renderer context on one HIP device (cudarender.cpp's gContext)."""

    def __init__(self, device=0, devices=None):
        """devices: a list of device ordinals -> one multi-device context
        (pm_config::n_devices: scene calls, render() and render_simple()
        only; photon shards + RCCL all-gather + 8-row bands per device)."""
        self.lib = load_library()
        h = ctypes.c_void_p()
        cfg = PMConfig(device=device)
        if devices is not None:
            self._devlist = (ctypes.c_int * len(devices))(*devices)
            cfg.n_devices = len(devices)
            cfg.devices = ctypes.cast(self._devlist, ctypes.POINTER(ctypes.c_int))
        rc = self.lib.pm_create(ctypes.byref(h), ctypes.byref(cfg))
        if rc != 0:
            raise PMError(rc, self.lib.pm_last_error(None).decode())
        self.h = h
        self.device = device
        self.devices = list(devices) if devices is not None else [device]
        self.width = self.height = 0
        self.pinhole = False
        self.camera = None  # the Camera of set_camera; width x height is then the sample raster

    def close(self):
        if getattr(self, "h", None):
            self.lib.pm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.pm_last_error(self.h).decode()
            if rc == PM_ERR_NO_PHOTONS:
                raise NoPhotonsError(rc, msg)
            raise PMError(rc, msg)

    # ---- scene (Scene.load_into protocol) ---------------------------------
    def add_material(self, mtype, rgb):
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_material(self.h, int(mtype), fptr(f32(rgb, 3)), ctypes.byref(out)))
        return out.value

    # textures (pm_add_texture_*): an operand is a texture id (int) or an rgb
    @staticmethod
    def _operand(op):
        if isinstance(op, (int, np.integer)):
            return int(op), None
        return -1, f32(op, 3)

    def add_texture_image(self, image, wrap="repeat", mapping=(1.0, 1.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
        """An image texture: image is (h, w, 3) float RGB, row 0 at v = 0; wrap a name of TEX_WRAPS or a
        PM_TEX_WRAP_* value; mapping = (su, sv, du, dv). Returns the texture id."""
        img = np.ascontiguousarray(np.asarray(image, dtype=np.float32))
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"expected an (h, w, 3) image, got shape {img.shape}")
        out = ctypes.c_int()
        w = TEX_WRAPS[wrap] if isinstance(wrap, str) else int(wrap)
        self._chk(self.lib.pm_add_texture_image(self.h, fptr(img), img.shape[1], img.shape[0], w, fptr(f32(mapping, 4)),
                                                fptr(f32(scale, 3)), ctypes.byref(out)))
        return out.value

    def add_texture_checker(self, tex1, tex2, mapping=(1.0, 1.0, 0.0, 0.0)):
        (t1, c1), (t2, c2) = self._operand(tex1), self._operand(tex2)
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_texture_checker(self.h, fptr(f32(mapping, 4)), t1, fptr(c1), t2, fptr(c2), ctypes.byref(out)))
        return out.value

    def add_texture_scale(self, tex1, tex2):
        (t1, c1), (t2, c2) = self._operand(tex1), self._operand(tex2)
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_texture_scale(self.h, t1, fptr(c1), t2, fptr(c2), ctypes.byref(out)))
        return out.value

    def add_material_textured(self, mtype, kd_tex):
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_material_textured(self.h, int(mtype), int(kd_tex), ctypes.byref(out)))
        return out.value

    def add_material_specular(self, mtype, kr, kt=(1.0, 1.0, 1.0), index=1.5):
        """A PM_MIRROR or PM_GLASS of the physical model (pm_add_material_specular). Returns the material id."""
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_material_specular(self.h, int(mtype), fptr(f32(kr, 3)), fptr(f32(kt, 3)), float(index),
                                                    ctypes.byref(out)))
        return out.value

    def record_albedo(self):
        """(n_records, 3): the factor pm_final applies to each record's indirect term
        (pm_download_record_albedo; scenes with a textured or physically specular material only)."""
        out = np.zeros((self.num_records(), 3), np.float32)
        self._chk(self.lib.pm_download_record_albedo(self.h, fptr(out), len(out)))
        return out

    def upload_record_albedo(self, rgb):
        rgb = f32(rgb, 3 * self.num_records())
        self._chk(self.lib.pm_upload_record_albedo(self.h, fptr(rgb), rgb.size // 3))

    def add_trimesh(self, P, idx, N=None, uv=None, material=0, light=-1):
        P = f32(P)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        N, uv = f32(N), f32(uv)
        self._chk(self.lib.pm_add_trimesh(self.h, fptr(P), P.size // 3, iptr(idx), idx.size // 3, fptr(N), fptr(uv),
                                          int(material), int(light)))

    def add_object_mesh(self, P, idx, N=None, uv=None, material=0, light=-1):
        """A mesh stored once in object space (pm_add_object_mesh); returns its object id."""
        P = f32(P)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        N, uv = f32(N), f32(uv)
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_object_mesh(self.h, fptr(P), P.size // 3, iptr(idx), idx.size // 3, fptr(N),
                                              fptr(uv), int(material), int(light), ctypes.byref(out)))
        return out.value

    def add_mesh_instance(self, obj, o2w, w2o):
        """One instance of an object mesh (pm_add_mesh_instance): affine row-major 4x4 and its inverse."""
        self._chk(self.lib.pm_add_mesh_instance(self.h, int(obj), fptr(f32(o2w, 16)), fptr(f32(w2o, 16))))

    def add_sphere(self, r, o2w, w2o, material, light=-1):
        self._chk(self.lib.pm_add_sphere(self.h, float(r), fptr(f32(o2w, 16)), fptr(f32(w2o, 16)), int(material),
                                         int(light)))

    def add_disk(self, o, x, y, z, inner, phimax, material, light=-1):
        self._chk(self.lib.pm_add_disk(self.h, fptr(f32(o, 3)), fptr(f32(x, 3)), fptr(f32(y, 3)), fptr(f32(z, 3)),
                                       float(inner), float(phimax), int(material), int(light)))

    def add_light_point(self, pos, I):
        self._chk(self.lib.pm_add_light_point(self.h, fptr(f32(pos, 3)), fptr(f32(I, 3))))

    def add_light_disk(self, o, p1, p2, n, Le, area, nsamples):
        self._chk(self.lib.pm_add_light_disk(self.h, fptr(f32(o, 3)), fptr(f32(p1, 3)), fptr(f32(p2, 3)),
                                             fptr(f32(n, 3)), fptr(f32(Le, 3)), float(area), int(nsamples)))

    def add_light_mesh(self, P, idx, Le, nsamples, reverse_orientation=False):
        """A triangle-mesh area light (pm_add_light_mesh); returns its light index. The visible
        geometry is the caller's: add_trimesh(P, idx, ..., light=<the index>)."""
        P = f32(P)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_light_mesh(self.h, fptr(P), P.size // 3, iptr(idx), idx.size // 3,
                                             int(bool(reverse_orientation)), fptr(f32(Le, 3)), int(nsamples),
                                             ctypes.byref(out)))
        return out.value

    def add_light_distant(self, to_light, L):
        """A distant light (pm_add_light_distant): radiance L from the direction to_light; returns its light index."""
        out = ctypes.c_int()
        self._chk(self.lib.pm_add_light_distant(self.h, fptr(f32(to_light, 3)), fptr(f32(L, 3)), ctypes.byref(out)))
        return out.value

    def set_pinhole(self, eye, fwd, right, up, W, H):
        self.width, self.height, self.pinhole, self.camera = int(W), int(H), True, None
        self._chk(self.lib.pm_set_pinhole(self.h, fptr(f32(eye, 3)), fptr(f32(fwd, 3)), fptr(f32(right, 3)),
                                          fptr(f32(up, 3)), int(W), int(H)))

    def set_eye_rays(self, rays, rand2d=None, n2d=0):
        rays = f32(rays)
        rand2d = f32(rand2d)
        self.width, self.height, self.pinhole, self.camera = rays.size // 6, 1, False, None
        self._chk(self.lib.pm_set_eye_rays(self.h, fptr(rays), rays.size // 6, fptr(rand2d), int(n2d)))

    def set_camera(self, eye, fwd, right, up, W, H, xsamples=1, ysamples=1, jitter=True, lens_radius=0.0,
                   focal_distance=0.0, sample_seed=0, filter="none", **filter_kw):
        """The supersampled thin-lens camera with its film (pm_set_camera). W x H is the image;
        the context then works on the (W xsamples) x (H ysamples) sample raster (self.width x
        self.height, as after set_pinhole at that size). filter: a Filter or the arguments of
        Filter.make ("none": render() returns the sample raster)."""
        cam = Camera()
        cam.eye[:], cam.fwd[:], cam.right[:], cam.up[:] = f32(eye, 3), f32(fwd, 3), f32(right, 3), f32(up, 3)
        cam.width, cam.height, cam.xsamples, cam.ysamples = int(W), int(H), int(xsamples), int(ysamples)
        cam.jitter, cam.lens_radius, cam.focal_distance = int(bool(jitter)), float(lens_radius), float(focal_distance)
        cam.sample_seed = int(sample_seed)
        cam.filter = Filter.make(filter, **filter_kw)
        self._chk(self.lib.pm_set_camera(self.h, ctypes.byref(cam)))
        self.width, self.height, self.pinhole, self.camera = cam.width * cam.xsamples, cam.height * cam.ysamples, True, cam

    def film(self, d_samples, d_image, stream=None):
        """pm_film: device float3 sample raster (width x height) -> device float3 image."""
        self._chk(self.lib.pm_film(self.h, ctypes.c_void_p(d_samples), ctypes.c_void_p(d_image), stream))

    def camera_rays(self, first=0, count=None, pass_=0):
        """(rays (count, 6), film_xy (count, 2)) of samples [first, first + count) of the sample
        raster in eye pass pass_ (0: the eye pass; k: eye_resample(k)), computed by the device
        function the eye pass calls (pm_camera_rays_pass)."""
        if count is None:
            count = self.width * self.height - first
        rays, xy = np.zeros((count, 6), np.float32), np.zeros((count, 2), np.float32)
        self._chk(self.lib.pm_camera_rays_pass(self.h, int(pass_), int(first), int(count), fptr(rays), fptr(xy)))
        return rays, xy

    def _out_shape(self):
        """(H, W) of what render() / render_simple() write for a device camera."""
        if self.camera is not None and self.camera.filter.type != PM_FILTER_NONE:
            return self.camera.height, self.camera.width
        return self.height, self.width

    def commit(self):
        self._chk(self.lib.pm_commit(self.h))

    # ---- whole render --------------------------------------------------------
    def render(self, params=None):
        params = params or RenderParams.defaults()
        oh, ow = self._out_shape()
        n = oh * ow if self.pinhole else self.num_records()
        out = np.zeros((n, 3), np.float32)
        st = Stats()
        self._chk(self.lib.pm_render(self.h, ctypes.byref(params), fptr(out), ctypes.byref(st)))
        if self.pinhole:
            out = out.reshape(oh, ow, 3)
        return out, st.as_dict()

    def render_resampled(self, params=None):
        """pm_render_resampled: a fresh eye sample of set_camera's jitter and lens every pass, one
        record per pixel (stochastic progressive photon mapping). Returns ((H, W, 3), stats)."""
        params = params or RenderParams.defaults()
        out = np.zeros((self.height * self.width, 3), np.float32)
        st = Stats()
        self._chk(self.lib.pm_render_resampled(self.h, ctypes.byref(params), fptr(out), ctypes.byref(st)))
        return out.reshape(self.height, self.width, 3), st.as_dict()

    def render_final_gather(self, params=None, n_gather=32):
        """pm_render_final_gather: the indirect light of every eye hit from n_gather cosine-sampled
        gather rays with a kNN estimate at their hits, not from the photon map at the hit itself."""
        params = params or RenderParams.defaults()
        oh, ow = self._out_shape()
        n = oh * ow if self.pinhole else self.num_records()
        out = np.zeros((n, 3), np.float32)
        st = Stats()
        self._chk(self.lib.pm_render_final_gather(self.h, ctypes.byref(params), int(n_gather), fptr(out), ctypes.byref(st)))
        if self.pinhole:
            out = out.reshape(oh, ow, 3)
        return out, st.as_dict()

    def render_simple(self, params=None):
        """SimpleRenderer (simplerender.cpp:18-103): direct light only."""
        params = params or RenderParams.simple_defaults()
        oh, ow = self._out_shape()
        n = oh * ow if self.pinhole else self.num_records()
        out = np.zeros((n, 3), np.float32)
        st = Stats()
        self._chk(self.lib.pm_render_simple(self.h, ctypes.byref(params), fptr(out), ctypes.byref(st)))
        if self.pinhole:
            out = out.reshape(oh, ow, 3)
        return out, st.as_dict()

    def simple_pass(self, params, d_out, stream=None):
        self._chk(self.lib.pm_simple_pass(self.h, ctypes.byref(params), d_out, stream))

    # ---- stages ---------------------------------------------------------------
    def eye_pass(self, params, stream=None):
        self._chk(self.lib.pm_eye_pass(self.h, ctypes.byref(params), stream))

    def eye_resample(self, params, pass_, stream=None):
        """pm_eye_resample: eye pass pass_ of a resampled render (0: eye_pass; k > 0: the records
        move to a fresh camera sample under their statistics, dl accumulates)."""
        self._chk(self.lib.pm_eye_resample(self.h, ctypes.byref(params), int(pass_), stream))

    def trace_photons(self, params, pass_index=0, path_begin=0, path_count=None, slot_path_base=0, stream=None):
        if path_count is None:
            path_count = params.paths_per_pass
        self._chk(self.lib.pm_trace_photons(self.h, ctypes.byref(params), int(pass_index), int(path_begin),
                                            int(path_count), int(slot_path_base), stream))

    def build_photon_map(self, params, n_slots=0, stream=None):
        self._chk(self.lib.pm_build_photon_map(self.h, ctypes.byref(params), int(n_slots), stream))

    def gather(self, params, stream=None):
        self._chk(self.lib.pm_gather(self.h, ctypes.byref(params), stream))

    def gather_range(self, params, rec_begin, rec_count, stream=None):
        self._chk(self.lib.pm_gather_range(self.h, ctypes.byref(params), int(rec_begin), int(rec_count), stream))

    def set_slot_buffer(self, d_ptr, n_slots):
        self._chk(self.lib.pm_set_slot_buffer(self.h, ctypes.c_void_p(d_ptr) if d_ptr else None, int(n_slots)))

    def gather_partial(self, params, d_partial, stream=None):
        self._chk(self.lib.pm_gather_partial(self.h, ctypes.byref(params), ctypes.c_void_p(d_partial), stream))

    def gather_split(self, params, d_count, d_flux, stream=None):
        self._chk(self.lib.pm_gather_split(self.h, ctypes.byref(params), d_count, d_flux, stream))

    def ppm_update_split(self, params, d_count, d_flux_chunk, v_begin, v_count, stream=None):
        self._chk(self.lib.pm_ppm_update_split(self.h, ctypes.byref(params), d_count, d_flux_chunk, int(v_begin),
                                               int(v_count), stream))

    def ppm_update_split_radius(self, params, d_count, d_ratio, stream=None):
        self._chk(self.lib.pm_ppm_update_split_radius(self.h, ctypes.byref(params), d_count, d_ratio, stream))

    def ppm_update_split_flux(self, params, d_ratio, d_flux_chunk, v_begin, v_count, stream=None):
        self._chk(self.lib.pm_ppm_update_split_flux(self.h, ctypes.byref(params), d_ratio, d_flux_chunk,
                                                    int(v_begin), int(v_count), stream))

    def ppm_update(self, params, d_partial, rec_begin, rec_count, stream=None):
        self._chk(self.lib.pm_ppm_update(self.h, ctypes.byref(params), ctypes.c_void_p(d_partial), int(rec_begin),
                                         int(rec_count), stream))

    def get_radius2(self, rec_begin, rec_count, d_out, stream=None):
        self._chk(self.lib.pm_get_radius2(self.h, int(rec_begin), int(rec_count), ctypes.c_void_p(d_out), stream))

    def set_radius2(self, d_in, rec_begin, rec_count, stream=None):
        self._chk(self.lib.pm_set_radius2(self.h, ctypes.c_void_p(d_in), int(rec_begin), int(rec_count), stream))

    def final(self, emitted, rec_begin, rec_count, d_out, stream=None):
        self._chk(self.lib.pm_final(self.h, float(emitted), int(rec_begin), int(rec_count), ctypes.c_void_p(d_out),
                                    stream))

    def final_gather_pass(self, params, n_gather, pass_=0, stream=None):
        """pm_final_gather_pass: n_gather gather rays per active record against the built photon
        buckets, their radiances added to the records' sums (pass_ 0 starts the sums)."""
        self._chk(self.lib.pm_final_gather_pass(self.h, ctypes.byref(params), int(n_gather), int(pass_), stream))

    def final_gather_resolve(self, rec_begin=0, rec_count=None):
        """pm_final_gather_resolve of records [rec_begin, rec_begin + rec_count) into a zeroed torch
        device buffer, returned on the host: the (H, W, 3) raster for pinhole and camera contexts
        (the call writes in raster order), else (rec_count, 3) in record order."""
        import torch
        n = self.num_records()
        if rec_count is None:
            rec_count = n - rec_begin
        rows = self.height * self.width if self.pinhole else rec_count
        d = torch.zeros((rows, 3), dtype=torch.float32, device=f"cuda:{self.device}")
        torch.cuda.synchronize()
        self._chk(self.lib.pm_final_gather_resolve(self.h, int(rec_begin), int(rec_count), ctypes.c_void_p(d.data_ptr()), None))
        self.synchronize()
        out = d.cpu().numpy()
        return out.reshape(self.height, self.width, 3) if self.pinhole else out

    def final_gather_rays(self, params, n_gather, pass_=0, first=0, count=None):
        """(count, 6) rays (o, d) of secondary records [first, first + count), by the device function
        final_gather_pass calls; all zero for a ray that is not traced (pm_final_gather_rays)."""
        if count is None:
            count = self.num_records() * int(n_gather) - first
        rays = np.zeros((count, 6), np.float32)
        self._chk(self.lib.pm_final_gather_rays(self.h, ctypes.byref(params), int(n_gather), int(pass_), int(first),
                                                int(count), fptr(rays)))
        return rays

    def gather_sum(self, n=None):
        """The final-gather sums A of the first n primary records, (n, 3) (pm_download_gather_sum)."""
        n = self.num_records() if n is None else int(n)
        out = np.zeros((n, 3), np.float32)
        self._chk(self.lib.pm_download_gather_sum(self.h, fptr(out), n))
        return out

    # ---- the caustic map of final gathering (pm_api.h pm_set_caustic_map) ----
    def set_caustic_map(self, on=True):
        """pm_set_caustic_map: trace_photons marks caustic photons (bit 1 of a slot's bits), and
        render_final_gather looks a map of them up at the eye hits. Off by default."""
        self._chk(self.lib.pm_set_caustic_map(self.h, int(bool(on))))

    def build_caustic_map(self, stream=None):
        """pm_build_caustic_map: the marked slots into a bucket set of their own (after build_photon_map)."""
        self._chk(self.lib.pm_build_caustic_map(self.h, stream))

    def caustic_gather(self, params, pass_=0, stream=None):
        """pm_caustic_gather: the kNN gather over the primary records against the caustic map."""
        self._chk(self.lib.pm_caustic_gather(self.h, ctypes.byref(params), int(pass_), stream))

    def caustic_map_count(self):
        n = int(self.lib.pm_caustic_map_count(self.h))
        if n < 0:
            raise PMError(1, "pm_caustic_map_count: no caustic map built")
        return n

    def caustic_slots(self):
        """The slot indices of the caustic map's photons in map order (pm_download_caustic_slots)."""
        out = np.zeros(self.caustic_map_count(), np.uint32)
        self._chk(self.lib.pm_download_caustic_slots(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(out)))
        return out

    def caustic_cell_start(self):
        """cell_start of the caustic map: cells + 1 words, the last one its photon count."""
        out = np.zeros(self.map_info()["cells"] + 1, np.uint32)
        self._chk(self.lib.pm_download_caustic_cell_start(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(out)))
        return out

    def caustic_radiance(self, n=None):
        """Lc of the first n primary records, (n, 3) (pm_download_caustic_radiance)."""
        n = self.num_records() if n is None else int(n)
        out = np.zeros((n, 3), np.float32)
        self._chk(self.lib.pm_download_caustic_radiance(self.h, fptr(out), n))
        return out

    def final_image(self, emitted):
        """pm_final over all records into a torch device buffer, returned on the
        host in the oracle's layout: (H, W, 3) raster for pinhole, else per ray."""
        import torch
        n = self.num_records()
        d = torch.empty((n, 3), dtype=torch.float32, device=f"cuda:{self.device}")
        torch.cuda.synchronize()
        self.final(emitted, 0, n, d.data_ptr())
        self.synchronize()
        out = d.cpu().numpy()
        if not self.pinhole:
            return out
        img = np.zeros((self.height * self.width, 3), np.float32)
        pix = self.record_pixels()
        ok = pix >= 0
        img[pix[ok]] = out[ok]
        return img.reshape(self.height, self.width, 3)

    # ---- buffers ----------------------------------------------------------------
    def num_records(self):
        return int(self.lib.pm_num_records(self.h))

    def record_pixels(self):
        n = self.num_records()
        if not self.pinhole:
            return np.arange(n, dtype=np.int64)
        return record_pixels(n, self.width, self.height)

    def reserve_slots(self, n):
        p = ctypes.c_void_p()
        self._chk(self.lib.pm_reserve_slots(self.h, int(n), ctypes.byref(p)))
        return p.value

    def download_slots(self, n):
        out = np.zeros(n, dtype=PHOTON_DTYPE)
        self._chk(self.lib.pm_download_slots(self.h, out.ctypes.data, n))
        return out

    def upload_slots(self, slots):
        slots = np.ascontiguousarray(slots, dtype=PHOTON_DTYPE)
        self._chk(self.lib.pm_upload_slots(self.h, slots.ctypes.data, len(slots)))

    def download_records(self):
        n = self.num_records()
        out = np.zeros(n, dtype=RECORD_DTYPE)
        self._chk(self.lib.pm_download_records(self.h, out.ctypes.data, n))
        return out

    def upload_records(self, recs):
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        self._chk(self.lib.pm_upload_records(self.h, recs.ctypes.data, len(recs)))

    def download_kdtree(self):
        n = int(self.lib.pm_kdtree_nodes(self.h))
        out = np.zeros(max(n, 0), dtype=PHOTON_DTYPE)
        if n > 0:
            self._chk(self.lib.pm_download_kdtree(self.h, out.ctypes.data, n))
        return out

    def set_record_view(self, active_only=True):
        """Index record-range calls by active records only (compacted); returns the view size."""
        n = ctypes.c_int64()
        self._chk(self.lib.pm_set_record_view(self.h, int(bool(active_only)), ctypes.byref(n)))
        return int(n.value)

    def final_view(self, emitted, v_begin, v_count, d_out, stream=None):
        self._chk(self.lib.pm_final_view(self.h, float(emitted), int(v_begin), int(v_count), ctypes.c_void_p(d_out),
                                         stream))

    def record_view_list(self, d_out, stream=None):
        self._chk(self.lib.pm_record_view_list(self.h, ctypes.c_void_p(d_out), stream))

    def set_stage_timing(self, stages="all"):
        """Stages that record HIP events: "all", "" (none) or e.g. "gather"."""
        self._chk(self.lib.pm_set_stage_timing(self.h, (stages or "").encode()))

    def set_counting(self, enabled=True):
        self._chk(self.lib.pm_set_counting(self.h, int(bool(enabled))))

    def gather_counters(self, full=False):
        """(visited, in_radius) or, with full=True, (visited, in_radius, bucket_rows, active_records)."""
        out = (ctypes.c_int64 * 4)()
        self._chk(self.lib.pm_gather_counters(self.h, out))
        vals = tuple(int(v) for v in out)
        return vals if full else vals[:2]

    def trace_counters(self):
        """(rays traced, BVH nodes entered, primitive tests, photons deposited) of the last
        trace_photons launched with counting on."""
        out = (ctypes.c_int64 * 4)()
        self._chk(self.lib.pm_trace_counters(self.h, out))
        return tuple(int(v) for v in out)

    def scene_info(self):
        """dict: triangles, disks, spheres, bvh_nodes, bvh_depth, mode ("bvh-hbm" | "bvh-lds" | "brute"), bytes."""
        out = (ctypes.c_int64 * 7)()
        self._chk(self.lib.pm_scene_info(self.h, out))
        v = [int(x) for x in out]
        return {"triangles": v[0], "disks": v[1], "spheres": v[2], "bvh_nodes": v[3], "bvh_depth": v[4],
                "mode": ("bvh-hbm", "bvh-lds", "brute", "bvh-instanced")[v[5]], "bytes": v[6]}

    SCENE_SECTIONS = {"refs": (0, np.uint32), "tri_geo": (1, np.float32), "tri_shade": (2, np.float32),
                      "tri_id": (3, np.uint32), "tri_info": (4, np.int32), "bvh4": (5, np.uint32),
                      "instances": (6, np.float32), "obj_tris": (7, np.float32),
                      "light_tris": (8, LIGHT_TRI_DTYPE), "light_cdf": (9, np.float32)}
    # textured scenes (empty otherwise): the texture records and per material its Kd texture; buffers of
    # their own, kept apart from the sections every scene has
    TEXTURE_SECTIONS = {"textures": (PM_SCENE_TEXTURES, TEX_REC_DTYPE), "mat_tex": (PM_SCENE_MAT_TEX, np.int32),
                        "mat_spec": (PM_SCENE_MAT_SPEC, np.float32)}  # 8 floats per material (pm_api.h)

    def scene_section(self, name):
        """One section of the committed scene blob as the kernels read it (pm_scene_section)."""
        sec, dt = self.SCENE_SECTIONS[name] if name in self.SCENE_SECTIONS else self.TEXTURE_SECTIONS[name]
        n = ctypes.c_int64()
        self._chk(self.lib.pm_scene_section(self.h, sec, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value // np.dtype(dt).itemsize, dtype=dt)
        if n.value:
            self._chk(self.lib.pm_scene_section(self.h, sec, out.ctypes.data, n.value, ctypes.byref(n)))
        return out

    def world_sphere(self):
        """The last commit's world sphere (PM_SCENE_WORLD_SPHERE; a host value, not a section of the
        scene blob): float32 centre x, y, z and radius, as the distant lights use it."""
        out = np.zeros(4, np.float32)
        n = ctypes.c_int64()
        self._chk(self.lib.pm_scene_section(self.h, PM_SCENE_WORLD_SPHERE, out.ctypes.data, out.nbytes, ctypes.byref(n)))
        assert n.value == out.nbytes
        return out

    def map_info(self):
        """dict: structure (PM_GATHER_*, -1 none), valid photons, slots, grid cells of the current photon map."""
        out = (ctypes.c_int64 * 4)()
        self._chk(self.lib.pm_map_info(self.h, out))
        v = [int(x) for x in out]
        return {"structure": v[0], "valid": v[1], "slots": v[2], "cells": v[3]}

    # ---- test hooks of the photon buckets, the tile list and the record view (read only) ----
    def map_grid(self):
        """dict: dims (dx, dy, dz), origin (float32 x 3) and inv_cs_bits of the built buckets' grid (pm_map_grid)."""
        dims, org, ib = (ctypes.c_int32 * 3)(), np.zeros(3, np.float32), ctypes.c_uint32()
        self._chk(self.lib.pm_map_grid(self.h, dims, fptr(org), ctypes.byref(ib)))
        return {"dims": tuple(int(d) for d in dims), "origin": org, "inv_cs_bits": int(ib.value)}

    def _map_words(self, fn):
        out = np.zeros(self.map_info()["cells"] + 1, np.uint32)
        self._chk(fn(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(out)))
        return out

    def map_counters(self):
        """The cells + 1 bucket counters (pm_download_map_counters): all zero after a build."""
        return self._map_words(self.lib.pm_download_map_counters)

    def photon_map(self):
        """(cell_start [cells + 1] uint32, ph_a [n, 4] float32, ph_b [n, 2, 4] float32) of the built buckets, n =
        cell_start[-1] photons in map order (pm_download_map_cell_start, pm_download_map_photons)."""
        cs = self._map_words(self.lib.pm_download_map_cell_start)
        n = min(int(cs[-1]), self.map_info()["slots"])  # never beyond what the build sized the arrays for
        a, b = np.zeros((n, 4), np.float32), np.zeros((n, 2, 4), np.float32)
        self._chk(self.lib.pm_download_map_photons(self.h, fptr(a), fptr(b), n))
        return cs, a, b

    def tile_list(self):
        """(the tile list, uint32; whether a gather's costs have reordered it) (pm_download_tile_list)."""
        n, srt = ctypes.c_int64(), ctypes.c_int()
        self._chk(self.lib.pm_download_tile_list(self.h, None, 0, ctypes.byref(n), ctypes.byref(srt)))
        out = np.zeros(max(int(n.value), 1), np.uint32)
        self._chk(self.lib.pm_download_tile_list(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(out),
                                                 ctypes.byref(n), ctypes.byref(srt)))
        return out[:int(n.value)], bool(srt.value)

    def record_view_size(self):
        n = ctypes.c_int64()
        self._chk(self.lib.pm_record_view_size(self.h, ctypes.byref(n)))
        return int(n.value)

    def trace_profile(self, reset=False):
        """k_trace phase cycles (profiling builds, lib/libpmhip_prof.so): dict of summed cycles."""
        out = (ctypes.c_int64 * 8)()
        self._chk(self.lib.pm_trace_profile(self.h, out, int(bool(reset))))
        keys = ("emit", "traverse", "shade", "compact_barrier", "exchange", "unused", "lifetime", "waves")
        return dict(zip(keys, (int(v) for v in out)))

    def synchronize(self):
        self._chk(self.lib.pm_synchronize(self.h))

    def timing_reset(self):
        self._chk(self.lib.pm_timing_reset(self.h))

    def timing_total(self, name):
        n, ms = ctypes.c_int64(), ctypes.c_double()
        self._chk(self.lib.pm_timing_total(self.h, name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        return int(n.value), ms.value

    def reset_records(self, params, stream=None):
        self._chk(self.lib.pm_reset_records(self.h, ctypes.byref(params), stream))

    def last_ms(self, name):
        ms = ctypes.c_double()
        self._chk(self.lib.pm_last_kernel_ms(self.h, name.encode(), ctypes.byref(ms)))
        return ms.value
