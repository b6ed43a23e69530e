"""ctypes mirrors of the POD types in include/pm_api.h (shared by the HIP
binding in hip.py and by the oracle binding in oracle/oracle.py)."""
import ctypes

import numpy as np

PM_OK = 0
PM_ERR_INVALID = 1
PM_ERR_HIP = 2
PM_ERR_NO_PHOTONS = 3
PM_ERR_NOMEM = 4

PM_MATTE, PM_MIRROR, PM_GLASS = 0, 1, 2
PM_LIGHT_POINT, PM_LIGHT_AREA_DISK = 1, 3
PM_LIGHT_AREA_MESH = 4  # ours: an emitting triangle mesh (pm_add_light_mesh)
PM_LIGHT_DISTANT = 6  # ours: pbrt-v2's distant light (pm_add_light_distant); 5 is kept for a spot light
PM_SCENE_WORLD_SPHERE = 10  # pm_scene_section: centre xyz, radius of the last commit's world sphere
PM_SCENE_TEXTURES, PM_SCENE_MAT_TEX = 11, 12  # pm_scene_section: the texture records, per material its Kd texture
PM_SCENE_MAT_SPEC = 13  # pm_scene_section: per material (Kr, index) (Kt, flag) of pm_add_material_specular
# wrap modes of an image texture (pm_add_texture_image)
PM_TEX_WRAP_REPEAT, PM_TEX_WRAP_BLACK, PM_TEX_WRAP_CLAMP = 0, 1, 2
TEX_WRAPS = {"repeat": PM_TEX_WRAP_REPEAT, "black": PM_TEX_WRAP_BLACK, "clamp": PM_TEX_WRAP_CLAMP}
TEX_SINGLE, TEX_CHECKER, TEX_SCALE = 0, 1, 2  # TexRec::kind
PM_REC_EXCEPTION, PM_REC_MISS, PM_REC_INVALID, PM_REC_BACKFACE = 0x1, 0x2, 0x4, 0x8
PM_REC_INACTIVE = PM_REC_EXCEPTION | PM_REC_MISS | PM_REC_INVALID
PM_GATHER_GRID, PM_GATHER_KDTREE = 0, 1
PM_ESTIMATOR_PPM, PM_ESTIMATOR_KNN = 0, 1
PM_KNN_MAX = 64
PM_FG_MAX = 256  # largest n_gather of pm_final_gather_pass
PM_ALL_LIGHTS = -1  # light_source_index: photon paths start on every light, picked by power
PM_PHOTON_MAX_RIGHT_CHILD = (1 << 29) - 1
# pm_filter::type; PM_FILM_TABLE: the film's weight table is 16 x 16 (pbrt ImageFilm)
PM_FILTER_NONE, PM_FILTER_BOX, PM_FILTER_TRIANGLE, PM_FILTER_GAUSSIAN, PM_FILTER_MITCHELL = 0, 1, 2, 3, 4
PM_FILM_TABLE = 16
FILTER_TYPES = {"none": PM_FILTER_NONE, "box": PM_FILTER_BOX, "triangle": PM_FILTER_TRIANGLE,
                "gaussian": PM_FILTER_GAUSSIAN, "mitchell": PM_FILTER_MITCHELL}

# pm_photon == reference CudaPhoton (photon_mapping/photonmapping.h:32-41), 40 B
PHOTON_DTYPE = np.dtype([("bits", "<u4"), ("p", "<f4", 3), ("alpha", "<f4", 3), ("wi", "<f4", 3)])
assert PHOTON_DTYPE.itemsize == 40
# pm_record (subset of RayTracingRecord, photonmapping.h:7-24), 64 B
RECORD_DTYPE = np.dtype([
    ("pos", "<f4", 3), ("flags", "<u4"), ("ns", "<f4", 3), ("material", "<i4"),
    ("flux", "<f4", 3), ("radius2", "<f4"), ("dl", "<f4", 3), ("photon_count", "<f4"),
])
assert RECORD_DTYPE.itemsize == 64
# one emitting triangle of a mesh light (PM_SCENE_LIGHT_TRIS; pm_scene_pod.h LightTri), 64 B
LIGHT_TRI_DTYPE = np.dtype([("p0", "<f4", 3), ("cdf", "<f4"), ("e1", "<f4", 4), ("e2", "<f4", 4), ("n", "<f4", 4)])
assert LIGHT_TRI_DTYPE.itemsize == 64
# one texture record (PM_SCENE_TEXTURES; pm_scene_pod.h TexRec), 128 B: an operand is a constant rgb
# (texel0 < 0) or an image (rgb = its scale, texel0 = its first texel, w, h, wrap, its mapping)
TEX_OPERAND_DTYPE = np.dtype([("rgb", "<f4", 3), ("texel0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("wrap", "<i4"),
                              ("pad", "<i4"), ("map", "<f4", 4)])
TEX_REC_DTYPE = np.dtype([("kind", "<i4"), ("pad", "<i4", 3), ("map", "<f4", 4), ("op", TEX_OPERAND_DTYPE, 2)])
assert TEX_OPERAND_DTYPE.itemsize == 48 and TEX_REC_DTYPE.itemsize == 128


class PMConfig(ctypes.Structure):
    """include/pm_api.h pm_config (32 B)."""
    _fields_ = [
        ("device", ctypes.c_int),
        ("n_devices", ctypes.c_int),
        ("devices", ctypes.POINTER(ctypes.c_int)),
        ("reserved", ctypes.c_int * 4),
    ]


class Filter(ctypes.Structure):
    """include/pm_api.h pm_filter (20 B): a = gaussian alpha / mitchell B, b = mitchell C."""
    _fields_ = [
        ("type", ctypes.c_int),
        ("xwidth", ctypes.c_float),
        ("ywidth", ctypes.c_float),
        ("a", ctypes.c_float),
        ("b", ctypes.c_float),
    ]

    # pbrt-v2's defaults per filter: (xwidth, ywidth, a, b)
    DEFAULTS = {PM_FILTER_NONE: (0.0, 0.0, 0.0, 0.0), PM_FILTER_BOX: (0.5, 0.5, 0.0, 0.0),
                PM_FILTER_TRIANGLE: (2.0, 2.0, 0.0, 0.0), PM_FILTER_GAUSSIAN: (2.0, 2.0, 2.0, 0.0),
                PM_FILTER_MITCHELL: (2.0, 2.0, 1.0 / 3.0, 1.0 / 3.0)}

    @classmethod
    def make(cls, kind="none", xwidth=None, ywidth=None, a=None, b=None):
        """kind: a name of FILTER_TYPES, a PM_FILTER_* value or a Filter; missing
        parameters take pbrt's defaults (ywidth: xwidth when only that is given)."""
        if isinstance(kind, cls):
            return kind
        t = FILTER_TYPES[kind] if isinstance(kind, str) else int(kind)
        d = cls.DEFAULTS.get(t, (0.0, 0.0, 0.0, 0.0))
        xw = d[0] if xwidth is None else xwidth
        yw = (d[1] if xwidth is None else xw) if ywidth is None else ywidth
        return cls(t, xw, yw, d[2] if a is None else a, d[3] if b is None else b)


class Camera(ctypes.Structure):
    """include/pm_api.h pm_camera (116 B)."""
    _fields_ = [
        ("eye", ctypes.c_float * 3),
        ("fwd", ctypes.c_float * 3),
        ("right", ctypes.c_float * 3),
        ("up", ctypes.c_float * 3),
        ("width", ctypes.c_int),
        ("height", ctypes.c_int),
        ("xsamples", ctypes.c_int),
        ("ysamples", ctypes.c_int),
        ("jitter", ctypes.c_int),
        ("lens_radius", ctypes.c_float),
        ("focal_distance", ctypes.c_float),
        ("sample_seed", ctypes.c_uint32),
        ("filter", Filter),
        ("reserved", ctypes.c_int * 4),
    ]


class RenderParams(ctypes.Structure):
    """pm_render_params; defaults are the reference's hard-coded constants."""
    _fields_ = [
        ("scene_epsilon", ctypes.c_float),
        ("initial_radius2", ctypes.c_float),
        ("ppm_alpha", ctypes.c_float),
        ("max_photon_count", ctypes.c_int),
        ("paths_per_pass", ctypes.c_int64),
        ("passes", ctypes.c_int),
        ("light_source_index", ctypes.c_int),
        ("max_specular_depth", ctypes.c_int),
        ("rng_seed", ctypes.c_uint32),
        ("light_rng_seed", ctypes.c_uint32),
        ("gather_structure", ctypes.c_int),
        ("estimator", ctypes.c_int),
        ("knn_lookup", ctypes.c_int),
        ("reserved", ctypes.c_int * 4),
    ]

    @classmethod
    def defaults(cls, **kw):
        p = cls()
        p.scene_epsilon = 0.1        # photonmappingrenderer.cpp:52
        p.initial_radius2 = 4.0      # raytracing.cu:123
        p.ppm_alpha = 0.7            # gathering.cu:115
        p.max_photon_count = 4       # photonmappingrenderer.cpp:183
        p.paths_per_pass = 512 * 512  # photonmappingrenderer.cpp:184-185
        p.passes = 1                 # photonmappingrenderer.cpp:38
        p.light_source_index = 0     # photonmappingrenderer.cpp:211 (PM_ALL_LIGHTS: every light)
        p.max_specular_depth = 10    # raytracing.cu:98
        p.rng_seed = 777             # cudarandom.h:15
        p.light_rng_seed = 2047
        p.gather_structure = PM_GATHER_GRID
        p.estimator = PM_ESTIMATOR_PPM
        p.knn_lookup = 50            # pbrt-v2 PhotonIntegrator "nused"
        return p._apply(kw)

    @classmethod
    def simple_defaults(cls, **kw):
        """the SimpleRenderer's constants: scene_epsilon 0.01 (simplerender.cpp:23)"""
        p = cls.defaults()
        p.scene_epsilon = 0.01
        return p._apply(kw)

    def _apply(self, kw):
        p = self
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"unknown render parameter {k!r}")
            setattr(p, k, v)
        return p


class Stats(ctypes.Structure):
    _fields_ = [
        ("paths_emitted", ctypes.c_int64),
        ("photons_valid", ctypes.c_int64),
        ("gather_points", ctypes.c_int64),
        ("nodes_visited", ctypes.c_int64),
        ("photons_in_radius", ctypes.c_int64),
        ("ms_eye", ctypes.c_double),
        ("ms_trace", ctypes.c_double),
        ("ms_build", ctypes.c_double),
        ("ms_gather", ctypes.c_double),
        ("ms_final", ctypes.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


def fptr(a):
    """float32 ndarray -> POINTER(c_float) (None passes NULL)."""
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def iptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def f32(a, n=None):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} floats, got {a.size}")
    return a


def record_pixels(n_records, width, height):
    """Pixel index of each record in the 8x8-tile order used by the pinhole
    camera (-1 for padding records). Mirrors rec_to_pixel in pm_device.h."""
    r = np.arange(n_records, dtype=np.int64)
    tile, lane = r >> 6, r & 63
    tiles_x = (width + 7) // 8
    px = (tile % tiles_x) * 8 + (lane & 7)
    py = (tile // tiles_x) * 8 + (lane >> 3)
    pix = py * width + px
    pix[(px >= width) | (py >= height)] = -1
    return pix
