"""rt3 — MI355X-native render path of Lut99/RayTracer-3, Python host mirror.

The package directory is ``raytracer-3_amd``; import it with
``importlib.import_module("raytracer-3_amd")`` (the hyphen rules out a plain ``import``).

This module is a ctypes binding over ``librt3hip.so`` (C ABI: ``include/rt3.h``) and mirrors the reference's
host interface for the render path, same names and argument meaning:

=====================================  ==========================================================
reference (C++)                        here
=====================================  ==========================================================
``RayTracer::initialize_renderer()``   :func:`initialize_renderer`  (Renderer.hpp:63)
``Renderer::prerender(entities)``      :meth:`HipRenderer.prerender` (Renderer.hpp:48)
``Renderer::render(camera)``           :meth:`HipRenderer.render`    (Renderer.hpp:50)
``ECS::create_triangle/sphere/object`` :func:`create_triangle` ...   (entities/*.hpp)
``Camera::update`` / ``get_frame``     :class:`Camera`               (camera/Camera.hpp)
``Frame::d/w/h/to_ppm``                :class:`Frame`                (camera/Frame.hpp)
=====================================  ==========================================================

There is no CPU fallback: if the HIP library is missing or no GPU is present, construction of the
renderer raises :class:`Fatal` (the reference's ``CppDebugger::Fatal`` convention, Main.cpp:305).
Nothing here imports ``oracle/``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT3_LIB_PATH", os.path.join(_HERE, "librt3hip.so"))      # override: A/B two builds

# --------------------------------------------------------------------------------------------------------
# wire structs (include/rt3.h)
# --------------------------------------------------------------------------------------------------------
GFACE = np.dtype([("v1", "<u4"), ("v2", "<u4"), ("v3", "<u4"), ("_p0", "<u4"),
                  ("normal", "<f4", 3), ("_p1", "<u4"), ("color", "<f4", 3), ("_p2", "<u4")])
MATERIAL = np.dtype([("rgb", "<f4", 3), ("param", "<f4"), ("kind", "<u4")])

MAT_FLAT, MAT_LAMBERT, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2, 3
# batched ray queries (rt3_intersect / rt3_occluded): rt3_ray (32 bytes) and rt3_hit (16 bytes)
RAY = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("_pad", "<u4")])
HIT = np.dtype([("t", "<f4"), ("kind", "<u4"), ("index", "<u4"), ("_pad", "<u4")])
HIT_NONE, HIT_FACE, HIT_SPHERE, HIT_INVALID = 0, 1, 2, 3
# first-hit AOVs (rt3_render_aov): rt3_aov (48 bytes)
AOV = np.dtype([("albedo", "<f4", 3), ("coverage", "<f4"), ("normal", "<f4", 3), ("depth", "<f4"), ("kind", "<u4"), ("index", "<u4"),
                ("_pad", "<u4", 2)])
# the temporal denoiser's per-pixel history (rt3_denoise_temporal): rt3_history (48 bytes)
HISTORY = np.dtype([("colour", "<f4", 3), ("length", "<f4"), ("moments", "<f4", 2), ("depth", "<f4"), ("_pad0", "<f4"),
                    ("normal", "<f4", 3), ("_pad1", "<f4")])
OCCLUDED_INVALID = 0xFFFFFFFF      # rt3_occluded's word for an invalid ray
FLAG_GAMMA2, FLAG_BLACK_BACKGROUND, FLAG_REFERENCE_PRIMARY, FLAG_VARIANCE = 1, 2, 4, 8
FLAG_ENV_SAMPLING = 16             # importance sampling of the environment map, one shadow ray per Lambert scatter
FLAG_LIGHT_SAMPLING = 32           # importance sampling of the emissive primitives, one shadow ray per Lambert scatter
REGROUP_SPHERES, REGROUP_MESH = 1, 2      # rt3_regroup's `what`
# the display transform (rt3_display): curve, transfer, flags of rt3_display_params
DISPLAY_CLAMP, DISPLAY_REINHARD, DISPLAY_FILMIC = 0, 1, 2
DISPLAY_LINEAR, DISPLAY_GAMMA2, DISPLAY_SRGB = 0, 1, 2
DISPLAY_AUTO_EXPOSURE = 1
DISPLAY_DARK = 0xFFFFFFFF          # rt3_debug_display_bin's word for a pixel below 2^-16
LENS_EQUIRECT = 1
LENS_FISHEYE = 2
LENS_ORTHO = 3
LENS_CUBE = 4
_LENS_MODELS = {"equirect": LENS_EQUIRECT, "fisheye": LENS_FISHEYE, "ortho": LENS_ORTHO, "cube": LENS_CUBE}
# rt3_lens: 80 bytes
LENS = np.dtype([("model", "<u4"), ("half_fov_turns", "<f4"), ("half_extent", "<f4", 2), ("origin", "<f4", 3), ("_pad0", "<f4"),
                 ("right", "<f4", 3), ("_pad1", "<f4"), ("up", "<f4", 3), ("_pad2", "<f4"), ("forward", "<f4", 3), ("_pad3", "<f4")])
_DISPLAY_CURVES = {"clamp": DISPLAY_CLAMP, "reinhard": DISPLAY_REINHARD, "filmic": DISPLAY_FILMIC}
_DISPLAY_TRANSFERS = {"linear": DISPLAY_LINEAR, "gamma2": DISPLAY_GAMMA2, "srgb": DISPLAY_SRGB}


class rt3_camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("horizontal", C.c_float * 3),
                ("vertical", C.c_float * 3), ("lower_left_corner", C.c_float * 3)]


class rt3_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("seed", C.c_uint32), ("flags", C.c_uint32), ("lens_radius", C.c_float), ("t_min", C.c_float),
                ("tile_rows", C.c_uint32), ("tile_index", C.c_uint32), ("tile_count", C.c_uint32)]


class rt3_stats(C.Structure):
    _fields_ = [("ray_casts", C.c_uint64), ("prim_tests", C.c_uint64), ("samples", C.c_uint64),
                ("trace_ms", C.c_float), ("total_ms", C.c_float), ("launches", C.c_uint32),
                ("n_spheres", C.c_uint32), ("n_faces", C.c_uint32), ("mfma_flop_per_instruction", C.c_uint32), ("mfma_instructions", C.c_uint64),
                ("exact_tests", C.c_uint64), ("filter_tests", C.c_uint64), ("bound_tests", C.c_uint64)]


class rt3_aov_chain_params(C.Structure):
    """rt3_aov_chain_params (16 bytes): how far rt3_render_aov_specular* follows mirrors and glass."""
    _fields_ = [("max_bounces", C.c_uint32), ("max_fuzz", C.c_float), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class rt3_ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("_pad", C.c_uint32)]


class rt3_hit(C.Structure):
    _fields_ = [("t", C.c_float), ("kind", C.c_uint32), ("index", C.c_uint32), ("_pad", C.c_uint32)]


def make_rays(origins, directions, t_max=np.inf):
    """Packs rays for HipRenderer.intersect / occluded: (N, 3) origins and directions (any length; each direction is
    normalised in float32) and t_max (a scalar or (N,)).  A zero or non-finite direction stays invalid."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("origins and directions differ in length")
    rays = np.zeros(len(o), RAY)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inv = np.float32(1.0) / np.sqrt(dd)
        rays["direction"] = d * inv[:, None]
    rays["origin"] = o
    rays["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), (len(o),))
    return rays


class rt3_gather_copy(C.Structure):
    _fields_ = [("dst_offset", C.c_uint64), ("src_offset", C.c_uint64), ("dst_pitch", C.c_uint64), ("src_pitch", C.c_uint64),
                ("row_bytes", C.c_uint64), ("rows", C.c_uint32)]


def gather_plan(params):
    """The copies rt3_gather_rows issues for a shard, as a list of rt3_gather_copy (pure arithmetic, no device)."""
    out = (rt3_gather_copy * 2)()
    n = lib().rt3_gather_plan(C.byref(params), out)
    if n < 0:
        raise Fatal("rt3_gather_plan: bad shard parameters")
    return [out[i] for i in range(n)]


class DENOISE_PARAMS(C.Structure):
    """rt3_denoise_params (16 bytes): a-trous passes, normal exponent, sigma_l, sigma_z."""
    _fields_ = [("iterations", C.c_uint32), ("normal_power", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_depth", C.c_float)]


class TEMPORAL_PARAMS(C.Structure):
    """rt3_temporal_params (32 bytes): the a-trous passes, the blend floors and the consistency tolerances."""
    _fields_ = [("spatial", DENOISE_PARAMS), ("alpha", C.c_float), ("moments_alpha", C.c_float), ("depth_tolerance", C.c_float),
                ("normal_tolerance", C.c_float)]


class ADAPTIVE_PARAMS(C.Structure):
    """rt3_adaptive_params (16 bytes): first-round samples, samples per later round, the relative standard error at which a pixel stops and
    the floor added to the mean it is relative to."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("threshold", C.c_float), ("dark", C.c_float)]


class RADIANCE_PARAMS(C.Structure):
    """rt3_radiance_params (24 bytes): ray casts per path, seed, flags (FLAG_BLACK_BACKGROUND, FLAG_ENV_SAMPLING, FLAG_LIGHT_SAMPLING), the sample range and t_min."""
    _fields_ = [("max_depth", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32), ("sample_begin", C.c_uint32),
                ("sample_count", C.c_uint32), ("t_min", C.c_float)]


class DISPLAY_PARAMS(C.Structure):
    """rt3_display_params (32 bytes): curve, transfer, flags, the auto-exposure's trims in 1/1024, exposure, key, white."""
    _fields_ = [("curve", C.c_uint32), ("transfer", C.c_uint32), ("flags", C.c_uint32), ("trim_low", C.c_uint32), ("trim_high", C.c_uint32),
                ("exposure", C.c_float), ("key", C.c_float), ("white", C.c_float)]


def display_params(curve="filmic", transfer="srgb", exposure=1.0, auto=False, key=0.18, white=4.0, trim_low=102, trim_high=51):
    """DISPLAY_PARAMS from names ("clamp" | "reinhard" | "filmic", "linear" | "gamma2" | "srgb") or the DISPLAY_* constants."""
    c = _DISPLAY_CURVES.get(curve, curve) if isinstance(curve, str) else curve
    t = _DISPLAY_TRANSFERS.get(transfer, transfer) if isinstance(transfer, str) else transfer
    if isinstance(c, str) or isinstance(t, str):
        raise Fatal("display: curve is clamp | reinhard | filmic, transfer is linear | gamma2 | srgb")
    return DISPLAY_PARAMS(int(c), int(t), DISPLAY_AUTO_EXPOSURE if auto else 0, int(trim_low), int(trim_high), float(exposure), float(key), float(white))


# rt3_exposure (16 bytes): the state of a sequence's eye adaptation — level, frames, the gain applied, a pad
EXPOSURE = np.dtype([("level", np.uint32), ("frames", np.uint32), ("gain", np.float32), ("_pad", np.uint32)])
EXPOSURE_MAX_LEVEL = 511 << 19


class DISPLAY_SEQUENCE_PARAMS(C.Structure):
    """rt3_display_sequence_params (64 bytes): rt3_display's parameters, the adaptation's two rates in 1/1024, the bloom's levels, threshold and
    intensity, three pad words."""
    _fields_ = [("display", DISPLAY_PARAMS), ("adapt_brighter", C.c_uint32), ("adapt_darker", C.c_uint32), ("bloom_levels", C.c_uint32),
                ("bloom_threshold", C.c_float), ("bloom_intensity", C.c_float), ("_pad", C.c_uint32 * 3)]


def display_sequence_params(curve="filmic", transfer="srgb", exposure=1.0, auto=False, key=0.18, white=4.0, trim_low=102, trim_high=51,
                            adapt=(256, 64), bloom=None):
    """DISPLAY_SEQUENCE_PARAMS: display_params' arguments, adapt = (brighter, darker) in 1/1024, bloom = None or (levels, threshold, intensity)."""
    levels, threshold, intensity = bloom if bloom is not None else (0, 1.0, 0.25)
    return DISPLAY_SEQUENCE_PARAMS(display_params(curve, transfer, exposure, auto, key, white, trim_low, trim_high), int(adapt[0]), int(adapt[1]),
                                   int(levels), float(threshold), float(intensity))


class rt3_lens(C.Structure):
    """rt3_lens (80 bytes): the model, the fisheye's half field of view in turns, the orthographic window's half extents, the origin and the
    orthonormal frame (right, up, forward), right x up = -forward."""
    _fields_ = [("model", C.c_uint32), ("half_fov_turns", C.c_float), ("half_extent", C.c_float * 2),
                ("origin", C.c_float * 3), ("_pad0", C.c_float), ("right", C.c_float * 3), ("_pad1", C.c_float),
                ("up", C.c_float * 3), ("_pad2", C.c_float), ("forward", C.c_float * 3), ("_pad3", C.c_float)]


def make_lens(model, origin, at, vup=(0.0, 1.0, 0.0), fov_deg=180.0, extent=(1.0, 1.0)):
    """An rt3_lens at `origin` that looks towards `at` with `vup` up (rt3_lens_look_at).  model: LENS_* or "equirect" | "fisheye" | "ortho" | "cube";
    fov_deg: the fisheye's whole field of view across the shorter image side; extent: the orthographic window's (width, height)."""
    m = _LENS_MODELS.get(model, model) if isinstance(model, str) else model
    if isinstance(m, str):
        raise Fatal("lens: model is equirect | fisheye | ortho | cube")
    lens = rt3_lens()
    o, a, u = _f3(origin), _f3(at), _f3(vup)
    lib().rt3_lens_look_at(C.byref(lens), int(m), o, a, u)
    lens.half_fov_turns = np.float32(fov_deg) / np.float32(720.0)
    lens.half_extent[0] = np.float32(extent[0]) * np.float32(0.5)
    lens.half_extent[1] = np.float32(extent[1]) * np.float32(0.5)
    return lens


def lens_ray(lens, params, x, y, s):
    """The lens law on the host (rt3_debug_lens_ray; no device): sample s of frame pixel (x, y) as one RAY record."""
    out = np.zeros(1, RAY)
    if lib().rt3_debug_lens_ray(C.byref(lens), C.byref(params), int(x), int(y), int(s), _p(out)) != 0:
        raise Fatal("rt3_debug_lens_ray: a lens the entry points refuse, or a pixel / sample outside the frame")
    return out[0]


def turns(c, s):
    """The angle of the vector (c, s) in turns, in [0, 1), as the inverse lens law computes it (rt3_debug_turns; no device): float32, NaN for
    (0, 0) and for non-finite input."""
    return np.float32(lib().rt3_debug_turns(float(np.float32(c)), float(np.float32(s))))


def lens_pixel(prev_lens, width, height, r, is_hit=True):
    """The inverse lens law on the host (rt3_debug_optic_pixel; no device): where r — a point relative to prev_lens's origin, or for a miss a
    direction — lies in prev_lens's width x height frame -> (x', y', zhat float32, face, valid).  valid False: no history.  An orthographic miss is
    not projected: x' and y' are NaN and valid is True."""
    out = np.zeros(3, np.float32)
    v = np.ascontiguousarray(r, np.float32).reshape(3)
    face, valid = C.c_uint32(0), C.c_uint32(0)
    if lib().rt3_debug_optic_pixel(C.byref(prev_lens), int(width), int(height), _p(v), 1 if is_hit else 0, _p(out), C.byref(face), C.byref(valid)) != 0:
        raise Fatal("rt3_debug_optic_pixel: a lens the entry points refuse for this frame, or a frame below 2 x 2")
    return out[0], out[1], out[2], int(face.value), bool(valid.value)


class Fatal(RuntimeError):
    """Mirror of CppDebugger::Fatal: every backend error is fatal (Main.cpp:305-308)."""


# every symbol include/rt3.h declares; tests check the library exports all of them
EXPORTS = [
    "rt3_create", "rt3_destroy", "rt3_last_error", "rt3_set_sample_storage_cap", "rt3_set_mesh", "rt3_set_spheres",
    "rt3_render", "rt3_render_device", "rt3_render_path", "rt3_render_path_device", "rt3_rows_owned",
    "rt3_row_of_local", "rt3_get_stats", "rt3_prerender_triangle", "rt3_sphere_face_count",
    "rt3_sphere_vertex_count", "rt3_prerender_sphere", "rt3_object_count", "rt3_prerender_object",
    "rt3_transfer_entity", "rt3_camera_update", "rt3_camera_look_at", "rt3_frame_ppm_bytes", "rt3_frame_to_ppm",
    "rt3_scene_three_spheres", "rt3_scene_weekend", "rt3_scene_stress", "rt3_scene_cornell", "rt3_hash_u32",
    "rt3_random_float", "rt3_debug_arith", "rt3_debug_force_plain_mode_r",
    "rt3_mesh_begin", "rt3_mesh_put", "rt3_mesh_sphere", "rt3_mesh_commit", "rt3_mesh_download",
    "rt3_render_path_range", "rt3_render_path_range_device", "rt3_accum_download", "rt3_accum_upload", "rt3_gather_rows",
    "rt3_stream", "rt3_synchronize", "rt3_device_alloc_words", "rt3_device_free", "rt3_device_read_words", "rt3_debug_force_brute",
    "rt3_abi_version", "rt3_debug_force_flat_filter", "rt3_gather_plan",
    "rt3_intersect", "rt3_occluded", "rt3_intersect_device", "rt3_occluded_device",
    "rt3_camera_rays", "rt3_camera_rays_device", "rt3_render_aov", "rt3_render_aov_device", "rt3_accum_resolve", "rt3_accum_resolve_device",
    "rt3_frame_pfm_bytes", "rt3_frame_to_pfm", "rt3_denoise", "rt3_denoise_device", "rt3_denoise_temporal", "rt3_denoise_temporal_device",
    "rt3_motion", "rt3_motion_device", "rt3_denoise_temporal_motion", "rt3_denoise_temporal_motion_device",
    "rt3_update_spheres", "rt3_update_spheres_device", "rt3_update_mesh", "rt3_update_mesh_device",
    "rt3_debug_primary_lists", "rt3_debug_ctr_table",
    "rt3_regroup", "rt3_regroup_device", "rt3_debug_group_order",
    "rt3_render_path_adaptive", "rt3_render_path_adaptive_device",
    "rt3_set_spheres_device", "rt3_set_mesh_device", "rt3_debug_sphere_plan", "rt3_debug_sphere_build",
    "rt3_radiance", "rt3_radiance_device",
    "rt3_set_environment", "rt3_set_environment_device", "rt3_clear_environment", "rt3_environment_size", "rt3_debug_environment_lookup",
    "rt3_debug_environment_sample", "rt3_debug_environment_table",
    "rt3_debug_light_sample", "rt3_debug_light_table",
    "rt3_display", "rt3_display_device", "rt3_debug_display_state", "rt3_debug_display_bin", "rt3_debug_display_gain", "rt3_debug_display_pixel",
    "rt3_debug_display_srgb_table",
    "rt3_display_sequence", "rt3_display_sequence_device", "rt3_debug_display_bloom", "rt3_debug_exposure_step", "rt3_debug_bloom",
    "rt3_lens_look_at", "rt3_lens_rays", "rt3_lens_rays_device", "rt3_render_lens", "rt3_render_lens_device", "rt3_render_lens_aov",
    "rt3_render_lens_aov_device", "rt3_debug_lens_ray",
    "rt3_denoise_temporal_optic", "rt3_denoise_temporal_optic_device", "rt3_motion_optic", "rt3_motion_optic_device", "rt3_debug_turns",
    "rt3_debug_optic_pixel",
    "rt3_set_texture", "rt3_set_texture_device", "rt3_clear_textures", "rt3_texture_size", "rt3_bind_sphere_textures",
    "rt3_bind_sphere_textures_device", "rt3_bind_mesh_textures", "rt3_bind_mesh_textures_device", "rt3_debug_texture_lookup",
    "rt3_debug_texture_sphere_uv", "rt3_debug_texture_face_uv",
    "rt3_render_aov_specular", "rt3_render_aov_specular_device", "rt3_render_lens_aov_specular", "rt3_render_lens_aov_specular_device",
    "rt3_debug_aov_bounce",
]
TEX_MAX_TEXTURES = 256   # RT3_TEX_MAX_TEXTURES: texture slots per context
TEX_MAX_SIDE = 8192      # RT3_TEX_MAX_SIDE
TEX_NONE = 0xFFFFFFFF    # RT3_TEX_NONE: a primitive without a texture
TEX_REPEAT, TEX_CLAMP = 0, 1
_TEX_WRAPS = {"repeat": TEX_REPEAT, "clamp": TEX_CLAMP, TEX_REPEAT: TEX_REPEAT, TEX_CLAMP: TEX_CLAMP}
ABI_VERSION = 3          # RT3_ABI_VERSION of include/rt3.h these bindings (the STATS / PARAMS struct layouts below) were written against

_lib = None


def lib():
    """Loads librt3hip.so (built in-tree by ``__graft_entry__.build()`` / ``make -C raytracer-3_amd``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Fatal("librt3hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                    "there is no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 under the same SONAME.  If torch is going to
    # be used in this process (device buffers, streams, RCCL) it has to be loaded first, or its later CUDA init fails
    # with "No HIP GPUs are available"; librt3hip.so then binds to the runtime that is already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, f32, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.c_int
    sigs = {
        "rt3_create": (vp, [i32]), "rt3_destroy": (None, [vp]), "rt3_last_error": (C.c_char_p, [vp]),
        "rt3_set_sample_storage_cap": (i32, [vp, u64]),
        "rt3_set_mesh": (i32, [vp, vp, u32, vp, u32, vp]), "rt3_set_spheres": (i32, [vp, vp, vp, u32]),
        "rt3_render": (i32, [vp, vp, u32, u32, vp]), "rt3_render_device": (i32, [vp, vp, u32, u32, vp, vp]),
        "rt3_render_path": (i32, [vp, vp, vp, vp]), "rt3_render_path_device": (i32, [vp, vp, vp, vp, vp]),
        "rt3_rows_owned": (u32, [vp]), "rt3_row_of_local": (u32, [vp, u32]), "rt3_get_stats": (i32, [vp, vp]),
        "rt3_prerender_triangle": (None, [vp, vp, vp, vp, vp, vp]),
        "rt3_sphere_face_count": (u32, [u32, u32]), "rt3_sphere_vertex_count": (u32, [u32, u32]),
        "rt3_prerender_sphere": (None, [vp, f32, u32, u32, vp, vp, vp]),
        "rt3_object_count": (i32, [C.c_char_p, vp, vp]),
        "rt3_prerender_object": (i32, [C.c_char_p, vp, f32, vp, vp, u32, vp, u32]),
        "rt3_transfer_entity": (None, [vp, vp, vp, vp, vp, u32, vp, u32]),
        "rt3_camera_update": (None, [vp, f32, f32, f32]), "rt3_camera_look_at": (None, [vp, vp, vp, vp, f32, f32, f32]),
        "rt3_frame_ppm_bytes": (u64, [vp, u32, u32, vp, u64]), "rt3_frame_to_ppm": (i32, [vp, u32, u32, C.c_char_p]),
        "rt3_scene_three_spheres": (u32, [vp, vp, u32]), "rt3_scene_weekend": (u32, [u32, vp, vp, u32]),
        "rt3_scene_stress": (u32, [u32, u32, vp, vp, u32]), "rt3_scene_cornell": (u32, [u32, vp, vp, vp, u32]),
        "rt3_hash_u32": (u32, [u32]), "rt3_random_float": (f32, [u32]),
        "rt3_debug_arith": (i32, [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_debug_force_plain_mode_r": (i32, [vp, i32]),
        "rt3_debug_primary_lists": (i32, [vp, vp, vp, vp, u64, vp, vp]), "rt3_debug_ctr_table": (u32, [vp, u32]),
        "rt3_mesh_begin": (i32, [vp, u32, u32]), "rt3_mesh_put": (i32, [vp, vp, u32, vp, u32, u32, u32]),
        "rt3_mesh_sphere": (i32, [vp, vp, f32, u32, u32, vp, u32, u32]), "rt3_mesh_commit": (i32, [vp, vp]),
        "rt3_mesh_download": (i32, [vp, vp, vp]),
        "rt3_render_path_range": (i32, [vp, vp, vp, u32, u32, vp]),
        "rt3_render_path_range_device": (i32, [vp, vp, vp, u32, u32, vp, vp]),
        "rt3_accum_download": (i32, [vp, vp, vp, vp]), "rt3_accum_upload": (i32, [vp, vp, vp, vp, vp, u32]),
        "rt3_gather_rows": (i32, [vp, vp, vp, vp, vp, vp]), "rt3_stream": (vp, [vp]), "rt3_synchronize": (i32, [vp]),
        "rt3_device_alloc_words": (vp, [vp, u64]), "rt3_device_free": (None, [vp, vp]),
        "rt3_device_read_words": (i32, [vp, vp, u64, vp]), "rt3_debug_force_brute": (i32, [vp, i32]),
        "rt3_abi_version": (u32, []), "rt3_debug_force_flat_filter": (i32, [vp, i32]), "rt3_gather_plan": (i32, [vp, vp]),
        "rt3_intersect": (i32, [vp, vp, u32, f32, vp]), "rt3_occluded": (i32, [vp, vp, u32, f32, vp]),
        "rt3_intersect_device": (i32, [vp, vp, u32, f32, vp, vp]), "rt3_occluded_device": (i32, [vp, vp, u32, f32, vp, vp]),
        "rt3_camera_rays": (i32, [vp, vp, vp, u32, u32, vp]), "rt3_camera_rays_device": (i32, [vp, vp, vp, u32, u32, vp, vp]),
        "rt3_render_aov": (i32, [vp, vp, vp, vp]), "rt3_render_aov_device": (i32, [vp, vp, vp, vp, vp]),
        "rt3_accum_resolve": (i32, [vp, vp]), "rt3_accum_resolve_device": (i32, [vp, vp, vp]),
        "rt3_frame_pfm_bytes": (u64, [vp, u32, u32, u32, u32, vp, u64]), "rt3_frame_to_pfm": (i32, [vp, u32, u32, u32, u32, C.c_char_p]),
        "rt3_denoise": (i32, [vp, u32, u32, vp, vp, vp, vp]), "rt3_denoise_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp]),
        "rt3_denoise_temporal": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_denoise_temporal_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_motion": (i32, [vp, u32, u32, vp, vp, vp, u32, vp, u32, vp]),
        "rt3_motion_device": (i32, [vp, u32, u32, vp, vp, vp, u32, vp, u32, vp, vp]),
        "rt3_denoise_temporal_motion": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_denoise_temporal_motion_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_update_spheres": (i32, [vp, vp, u32]), "rt3_update_spheres_device": (i32, [vp, vp, u32, vp]),
        "rt3_update_mesh": (i32, [vp, vp, vp, u32]), "rt3_update_mesh_device": (i32, [vp, vp, vp, u32, vp]),
        "rt3_regroup": (i32, [vp, u32]), "rt3_regroup_device": (i32, [vp, u32, vp]), "rt3_debug_group_order": (i32, [vp, u32, vp, u64, vp]),
        "rt3_render_path_adaptive": (i32, [vp, vp, vp, vp, vp, vp]), "rt3_render_path_adaptive_device": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "rt3_set_spheres_device": (i32, [vp, vp, vp, u32, vp]), "rt3_set_mesh_device": (i32, [vp, vp, u32, vp, u32, vp, vp]),
        "rt3_debug_sphere_plan": (u32, [vp, u32, vp, vp]), "rt3_debug_sphere_build": (i32, [vp, vp, vp, vp]),
        "rt3_radiance": (i32, [vp, vp, vp, u32, vp, vp]), "rt3_radiance_device": (i32, [vp, vp, vp, u32, vp, vp, vp]),
        "rt3_set_environment": (i32, [vp, vp, u32]), "rt3_set_environment_device": (i32, [vp, vp, u32, vp]),
        "rt3_clear_environment": (i32, [vp]), "rt3_environment_size": (u32, [vp]),
        "rt3_debug_environment_lookup": (i32, [vp, u32, vp, vp]),
        "rt3_debug_environment_sample": (i32, [vp, u32, u32, u32, vp, vp, vp]), "rt3_debug_environment_table": (i32, [vp, vp, vp, u64, vp]),
        "rt3_debug_light_sample": (i32, [vp, u32, vp, u32, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]),
        "rt3_debug_light_table": (i32, [vp, vp, vp, u64, vp]),
        "rt3_display": (i32, [vp, u32, u32, vp, vp, vp]), "rt3_display_device": (i32, [vp, u32, u32, vp, vp, vp, vp]),
        "rt3_debug_display_state": (i32, [vp, vp, vp, vp]), "rt3_debug_display_bin": (i32, [vp, vp]),
        "rt3_debug_display_gain": (i32, [vp, vp, vp]), "rt3_debug_display_pixel": (i32, [vp, f32, vp, vp]),
        "rt3_debug_display_srgb_table": (i32, [vp]),
        "rt3_display_sequence": (i32, [vp, u32, u32, vp, vp, vp, vp, vp]),
        "rt3_display_sequence_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp]),
        "rt3_debug_display_bloom": (i32, [vp, vp, vp, u64, vp, vp]), "rt3_debug_exposure_step": (i32, [vp, vp, vp, vp]),
        "rt3_debug_bloom": (i32, [u32, u32, vp, f32, f32, u32, vp, vp]),
        "rt3_lens_look_at": (None, [vp, u32, vp, vp, vp]),
        "rt3_lens_rays": (i32, [vp, vp, vp, u32, u32, vp]), "rt3_lens_rays_device": (i32, [vp, vp, vp, u32, u32, vp, vp]),
        "rt3_render_lens": (i32, [vp, vp, vp, u32, u32, vp]), "rt3_render_lens_device": (i32, [vp, vp, vp, u32, u32, vp, vp]),
        "rt3_render_lens_aov": (i32, [vp, vp, vp, vp]), "rt3_render_lens_aov_device": (i32, [vp, vp, vp, vp, vp]),
        "rt3_debug_lens_ray": (i32, [vp, vp, u32, u32, u32, vp]),
        "rt3_denoise_temporal_optic": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_denoise_temporal_optic_device": (i32, [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt3_motion_optic": (i32, [vp, u32, u32, vp, vp, vp, u32, vp, u32, vp]),
        "rt3_motion_optic_device": (i32, [vp, u32, u32, vp, vp, vp, u32, vp, u32, vp, vp]),
        "rt3_debug_turns": (f32, [f32, f32]), "rt3_debug_optic_pixel": (i32, [vp, u32, u32, vp, u32, vp, vp, vp]),
        "rt3_set_texture": (i32, [vp, u32, vp, u32, u32, u32]), "rt3_set_texture_device": (i32, [vp, u32, vp, u32, u32, u32, vp]),
        "rt3_clear_textures": (i32, [vp]), "rt3_texture_size": (i32, [vp, u32, vp, vp, vp]),
        "rt3_bind_sphere_textures": (i32, [vp, vp, u32]), "rt3_bind_sphere_textures_device": (i32, [vp, vp, u32, vp]),
        "rt3_bind_mesh_textures": (i32, [vp, vp, vp, u32]), "rt3_bind_mesh_textures_device": (i32, [vp, vp, vp, u32, vp]),
        "rt3_debug_texture_lookup": (i32, [vp, u32, u32, u32, vp, vp]), "rt3_debug_texture_sphere_uv": (i32, [vp, vp]),
        "rt3_debug_texture_face_uv": (i32, [vp, vp, vp, vp, vp, vp]),
        "rt3_render_aov_specular": (i32, [vp, vp, vp, vp, vp]), "rt3_render_aov_specular_device": (i32, [vp, vp, vp, vp, vp, vp]),
        "rt3_render_lens_aov_specular": (i32, [vp, vp, vp, vp, vp]), "rt3_render_lens_aov_specular_device": (i32, [vp, vp, vp, vp, vp, vp]),
        "rt3_debug_aov_bounce": (i32, [vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.rt3_abi_version() != ABI_VERSION:
        raise Fatal("%s reports ABI version %d, these bindings were written against %d (include/rt3.h: RT3_ABI_VERSION)"
                    % (LIB_PATH, L.rt3_abi_version(), ABI_VERSION))
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _cube_rgba(cube):
    """(6, N, N, 3 | 4) -> contiguous float32 (6, N, N, 4), the layout rt3_set_environment takes (the fourth channel is ignored: 0 when absent)."""
    a = np.asarray(cube, np.float32)
    if a.ndim != 4 or a.shape[0] != 6 or a.shape[1] != a.shape[2] or a.shape[3] not in (3, 4) or a.shape[1] < 1:
        raise Fatal("an environment map is an array of shape (6, N, N, 3) or (6, N, N, 4)")
    if a.shape[3] == 3:
        a = np.concatenate([a, np.zeros(a.shape[:3] + (1,), np.float32)], axis=3)
    return np.ascontiguousarray(a)


def environment_lookup(cube, d):
    """rt3_debug_environment_lookup, the environment map's lookup law in C on the host: float32 (3,) for one direction, (K, 3) for K."""
    rgba = _cube_rgba(cube)
    dirs = np.ascontiguousarray(np.asarray(d, np.float32).reshape(-1, 3))
    out = np.zeros((len(dirs), 3), np.float32)
    fn = lib().rt3_debug_environment_lookup
    for k in range(len(dirs)):
        if fn(_p(rgba), rgba.shape[1], C.c_void_p(dirs.ctypes.data + 12 * k), C.c_void_p(out.ctypes.data + 12 * k)) != 0:
            raise Fatal("rt3_debug_environment_lookup refused its arguments (1 <= N <= 2048)")
    return out[0] if np.ndim(d) == 1 else out


def _image_rgba(image):
    """(H, W, 3 | 4) -> contiguous float32 (H, W, 4), the layout rt3_set_texture takes (row 0 on top; the fourth channel is ignored: 0 when absent)."""
    a = np.asarray(image, np.float32)
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise Fatal("a texture is an array of shape (H, W, 3) or (H, W, 4)")
    if a.shape[2] == 3:
        a = np.concatenate([a, np.zeros(a.shape[:2] + (1,), np.float32)], axis=2)
    return np.ascontiguousarray(a)


def _torch_word_dtypes():
    import torch
    return tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)


def _tex_wrap(wrap):
    if wrap not in _TEX_WRAPS:
        raise Fatal("wrap is 'repeat' or 'clamp'")
    return _TEX_WRAPS[wrap]


def texture_lookup(image, uv, wrap="repeat"):
    """rt3_debug_texture_lookup, the texture lookup law in C on the host: image (H, W, 3 | 4), uv (2,) or (K, 2) -> float32 (3,) or (K, 3)."""
    rgba = _image_rgba(image)
    q = np.ascontiguousarray(np.asarray(uv, np.float32).reshape(-1, 2))
    out = np.zeros((len(q), 3), np.float32)
    fn = lib().rt3_debug_texture_lookup
    for k in range(len(q)):
        if fn(_p(rgba), rgba.shape[1], rgba.shape[0], _tex_wrap(wrap), C.c_void_p(q.ctypes.data + 8 * k), C.c_void_p(out.ctypes.data + 12 * k)) != 0:
            raise Fatal("rt3_debug_texture_lookup refused its arguments (1 <= W, H <= 8192, W * H <= 2^26)")
    return out[0] if np.ndim(uv) == 1 else out


def texture_sphere_uv(n):
    """rt3_debug_texture_sphere_uv, a sphere's (u, v) from its unit outward normal in C on the host: n (3,) or (K, 3) -> float32 (2,) or (K, 2)."""
    q = np.ascontiguousarray(np.asarray(n, np.float32).reshape(-1, 3))
    out = np.zeros((len(q), 2), np.float32)
    fn = lib().rt3_debug_texture_sphere_uv
    for k in range(len(q)):
        fn(C.c_void_p(q.ctypes.data + 12 * k), C.c_void_p(out.ctypes.data + 8 * k))
    return out[0] if np.ndim(n) == 1 else out


def texture_face_uv(p1, p2, p3, uv6, p):
    """rt3_debug_texture_face_uv, a face's (u, v) at the point p in C on the host: vertices (3,), uv6 (6,), p (3,) or (K, 3) -> float32 (2,) or (K, 2)."""
    a, b, c = (np.ascontiguousarray(np.asarray(x, np.float32).reshape(3)) for x in (p1, p2, p3))
    t = np.ascontiguousarray(np.asarray(uv6, np.float32).reshape(6))
    q = np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 3))
    out = np.zeros((len(q), 2), np.float32)
    fn = lib().rt3_debug_texture_face_uv
    for k in range(len(q)):
        fn(_p(a), _p(b), _p(c), _p(t), C.c_void_p(q.ctypes.data + 12 * k), C.c_void_p(out.ctypes.data + 8 * k))
    return out[0] if np.ndim(p) == 1 else out


def environment_sample(cube, base, depth):
    """rt3_debug_environment_sample, the map's sampling table and sampling law in C on the host: what a Lambert scatter of a path
    with RNG base `base` at depth `depth` draws under FLAG_ENV_SAMPLING.  Scalars give (cell, float32 direction (3,), float32 pdf), arrays of K
    give (uint32 (K,), (K, 3), (K,)).  A map whose table is empty (nothing to sample) gives cell 0xFFFFFFFF, direction 0 and pdf 0."""
    rgba = _cube_rgba(cube)
    b = np.asarray(base, np.uint32).reshape(-1)
    d = np.broadcast_to(np.asarray(depth, np.uint32).reshape(-1), b.shape)
    cell = np.zeros(len(b), np.uint32)
    dirs = np.zeros((len(b), 3), np.float32)
    pdf = np.zeros(len(b), np.float32)
    fn = lib().rt3_debug_environment_sample
    for k in range(len(b)):
        if fn(_p(rgba), rgba.shape[1], int(b[k]), int(d[k]), C.c_void_p(cell.ctypes.data + 4 * k), C.c_void_p(dirs.ctypes.data + 12 * k),
              C.c_void_p(pdf.ctypes.data + 4 * k)) != 0:
            raise Fatal("rt3_debug_environment_sample refused its arguments (1 <= N <= 2048)")
    return (int(cell[0]), dirs[0], pdf[0]) if np.ndim(base) == 0 else (cell, dirs, pdf)


def light_sample(faces, verts, face_materials, center_radius, sphere_materials, base, depth):
    """rt3_debug_light_sample, the emitters' sampling table and sampling law in C on the host: what a Lambert scatter of a path with
    RNG base `base` at depth `depth` draws under FLAG_LIGHT_SAMPLING in the scene of these faces (GFACE, verts (n, 4), one MATERIAL per face) and
    spheres ((n, 4) centre and radius, one MATERIAL each); None or empty arrays for a class the scene lacks.  Scalars give (light, float32 point
    (3,), float32 light normal (3,), float32 area, float32 pl), arrays of K give (uint32 (K,), (K, 3), (K, 3), (K,), (K,)).  A table that is empty
    (no emitter) gives light 0xFFFFFFFF and zeros."""
    f = np.ascontiguousarray(faces if faces is not None else np.zeros(0, GFACE))
    v = np.ascontiguousarray(verts if verts is not None else np.zeros((0, 4)), np.float32).reshape(-1, 4)
    fm = np.ascontiguousarray(face_materials if face_materials is not None else np.zeros(0, MATERIAL))
    cr = np.ascontiguousarray(center_radius if center_radius is not None else np.zeros((0, 4)), np.float32).reshape(-1, 4)
    sm = np.ascontiguousarray(sphere_materials if sphere_materials is not None else np.zeros(0, MATERIAL))
    if f.dtype != GFACE or fm.dtype != MATERIAL or sm.dtype != MATERIAL or len(fm) != len(f) or len(sm) != len(cr):
        raise Fatal("light_sample: GFACE faces with one MATERIAL each, (n, 4) spheres with one MATERIAL each")
    b = np.asarray(base, np.uint32).reshape(-1)
    d = np.broadcast_to(np.asarray(depth, np.uint32).reshape(-1), b.shape)
    light = np.zeros(len(b), np.uint32)
    point = np.zeros((len(b), 3), np.float32)
    normal = np.zeros((len(b), 3), np.float32)
    area = np.zeros(len(b), np.float32)
    pl = np.zeros(len(b), np.float32)
    fn = lib().rt3_debug_light_sample
    for k in range(len(b)):
        if fn(_p(f) if len(f) else None, len(f), _p(v) if len(v) else None, len(v), _p(fm) if len(f) else None, _p(cr) if len(cr) else None,
              _p(sm) if len(cr) else None, len(cr), int(b[k]), int(d[k]), C.c_void_p(light.ctypes.data + 4 * k), C.c_void_p(point.ctypes.data + 12 * k),
              C.c_void_p(normal.ctypes.data + 12 * k), C.c_void_p(area.ctypes.data + 4 * k), C.c_void_p(pl.ctypes.data + 4 * k)) != 0:
            raise Fatal("rt3_debug_light_sample refused its arguments (a face index out of range?)")
    return (int(light[0]), point[0], normal[0], area[0], pl[0]) if np.ndim(base) == 0 else (light, point, normal, area, pl)


def display_bin(rgb):
    """rt3_debug_display_bin, the auto-exposure's histogram bin in C on the host: (3,) -> int, (K, 3) -> uint32 (K,); 0 .. 511, or
    DISPLAY_DARK for a pixel whose luminance is below 2^-16."""
    c = np.ascontiguousarray(np.asarray(rgb, np.float32).reshape(-1, 3))
    out = np.zeros(len(c), np.uint32)
    fn = lib().rt3_debug_display_bin
    for k in range(len(c)):
        if fn(C.c_void_p(c.ctypes.data + 12 * k), C.c_void_p(out.ctypes.data + 4 * k)) != 0:
            raise Fatal("rt3_debug_display_bin refused its arguments")
    return int(out[0]) if np.ndim(rgb) == 1 else out


def display_gain(hist, exposure=1.0, key=0.18, trim_low=102, trim_high=51):
    """rt3_debug_display_gain, the auto-exposure's gain of a histogram of 512 uint32 bins in C on the host -> float32."""
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (512,):
        raise Fatal("display_gain: the histogram has 512 bins")
    p = display_params(exposure=exposure, key=key, trim_low=trim_low, trim_high=trim_high)
    g = C.c_float(0.0)
    if lib().rt3_debug_display_gain(_p(h), C.byref(p), C.byref(g)) != 0:
        raise Fatal("rt3_debug_display_gain refused its arguments (exposure and key finite and > 0, trim_low + trim_high <= 1023)")
    return np.float32(g.value)


def display_pixel(rgb, gain, curve="filmic", transfer="srgb", white=4.0):
    """rt3_debug_display_pixel, one pixel through the gain, the curve and the transfer in C on the host: (3,) -> int, (K, 3) ->
    uint32 (K,) words 0xFF | B << 8 | G << 16 | R << 24."""
    c = np.ascontiguousarray(np.asarray(rgb, np.float32).reshape(-1, 3))
    out = np.zeros(len(c), np.uint32)
    p = display_params(curve, transfer, white=white)
    fn = lib().rt3_debug_display_pixel
    for k in range(len(c)):
        if fn(C.c_void_p(c.ctypes.data + 12 * k), C.c_float(gain), C.byref(p), C.c_void_p(out.ctypes.data + 4 * k)) != 0:
            raise Fatal("rt3_debug_display_pixel refused its arguments (white >= 2^-10)")
    return int(out[0]) if np.ndim(rgb) == 1 else out


def display_srgb_table():
    """rt3_debug_display_srgb_table: the 4096 bytes the sRGB transfer looks up, uint8 (4096,)."""
    out = np.zeros(4096, np.uint8)
    if lib().rt3_debug_display_srgb_table(_p(out)) != 0:
        raise Fatal("rt3_debug_display_srgb_table failed")
    return out


def exposure_step(prev, hist, params):
    """rt3_debug_exposure_step, the adaptation law in C on the host: the EXPOSURE record after a frame with this histogram of 512
    uint32 bins under params (a DISPLAY_SEQUENCE_PARAMS); prev: None or the EXPOSURE record before."""
    h = np.ascontiguousarray(hist, np.uint32).reshape(-1)
    if h.size != 512:
        raise Fatal("exposure_step: the histogram has 512 bins")
    before = np.array(prev, EXPOSURE).reshape(1) if prev is not None else None
    out = np.zeros(1, EXPOSURE)
    if lib().rt3_debug_exposure_step(_p(before), _p(h), C.byref(params), _p(out)) != 0:
        raise Fatal("rt3_debug_exposure_step refused its arguments (rates 1 .. 1024, prev only with auto-exposure, prev.level <= 511 << 19)")
    return out[0]


def bloom_plane(colour, gain, threshold, levels):
    """rt3_debug_bloom, the bloom law in C on the host, serially: float32 (H, W, 4) -> (U_1 float32 (H_1, W_1, 4), B float32
    (H, W, 4)) under the given gain, threshold and number of levels (1 .. 8)."""
    c = np.ascontiguousarray(colour, np.float32)
    if c.ndim != 3 or c.shape[2] != 4:
        raise Fatal("bloom_plane: colour must be float32 (H, W, 4)")
    h, w = c.shape[:2]
    u1 = np.zeros(((h + 1) // 2, (w + 1) // 2, 4), np.float32)
    b = np.zeros((h, w, 4), np.float32)
    if lib().rt3_debug_bloom(w, h, _p(c), float(np.float32(gain)), float(np.float32(threshold)), int(levels), _p(u1), _p(b)) != 0:
        raise Fatal("rt3_debug_bloom refused its arguments (levels 1 .. 8, a finite threshold >= 0, 1 .. 2^26 pixels)")
    return u1, b


def cube_from_equirect(image, n):
    """A latitude-longitude image (H, W, 3 | 4; row 0 is +Y, the centre column is -Z, longitude grows towards +X) -> a cube map (6, n, n, 4)
    float32 for set_environment: every texel centre's direction — the inverse of the lookup law's face coordinates — is looked up bilinearly in the
    image (float64 inside; columns wrap around, rows clamp at the poles)."""
    img = np.asarray(image, np.float64)
    if img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1 or n < 1:
        raise Fatal("cube_from_equirect takes an image (H, W, 3 | 4) and n >= 1")
    h, w = img.shape[:2]
    c = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0          # sc / m (columns) and tc / m (rows) of the texel centres
    sc, tc = np.meshgrid(c, c)                                           # [row j, column i]
    one = np.ones_like(sc)
    faces = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    out = np.zeros((6, n, n, 4), np.float32)
    for f, (x, y, z) in enumerate(faces):
        r = np.sqrt(x * x + y * y + z * z)
        lon = np.arctan2(x, -z)                                          # 0 at -Z, +pi/2 at +X
        lat = np.arcsin(np.clip(y / r, -1.0, 1.0))                       # +pi/2 at +Y
        fx = (lon / (2.0 * np.pi) + 0.5) * w - 0.5
        fy = (0.5 - lat / np.pi) * h - 0.5
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = (fx - x0)[..., None], (fy - y0)[..., None]
        xa, xb = x0.astype(np.int64) % w, (x0.astype(np.int64) + 1) % w
        ya, yb = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
        top = img[ya, xa, :3] * (1.0 - wx) + img[ya, xb, :3] * wx
        bot = img[yb, xa, :3] * (1.0 - wx) + img[yb, xb, :3] * wx
        out[f, :, :, :3] = (top * (1.0 - wy) + bot * wy).astype(np.float32)
    return out


def _f3(v):
    return (C.c_float * 3)(*[float(np.float32(x)) for x in v])


# --------------------------------------------------------------------------------------------------------
# Frame / Camera  (src/lib/camera/Frame.hpp:41-82, Camera.hpp:25-68)
# --------------------------------------------------------------------------------------------------------
class Frame:
    """uint32 RGBA8 frame, row 0 on top, word = 0xFF | B<<8 | G<<16 | R<<24 (SequentialRenderer.cpp:297)."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.data = np.zeros((self.height, self.width), np.uint32)

    def w(self):
        return self.width

    def h(self):
        return self.height

    def d(self):
        return self.data

    def ppm_bytes(self):
        """Exactly the bytes Frame::to_ppm writes (Frame.cpp:125-143)."""
        need = lib().rt3_frame_ppm_bytes(_p(self.data), self.width, self.height, None, 0)
        buf = np.zeros(need, np.uint8)
        lib().rt3_frame_ppm_bytes(_p(self.data), self.width, self.height, _p(buf), need)
        return buf.tobytes()

    def to_ppm(self, path):
        if lib().rt3_frame_to_ppm(_p(self.data), self.width, self.height, os.fsencode(path)) != 0:
            raise Fatal("Could not open '%s'" % path)

    def rgb(self):
        """(h, w, 3) uint8 view of the frame as PPM/PNG would show it."""
        d = self.data
        return np.stack([(d >> 24) & 0xFF, (d >> 16) & 0xFF, (d >> 8) & 0xFF], axis=-1).astype(np.uint8)


def pfm_bytes(image):
    """rt3_frame_pfm_bytes of a float32 image, row 0 on top: (h, w) -> "Pf", (h, w, 3) -> "PF".  The image may be a strided view of a wider
    record (e.g. ``aov["albedo"]`` of an AOV frame) as long as its pixels are evenly spaced and its rows contiguous."""
    a = np.asarray(image)
    if a.dtype != np.float32 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("pfm_bytes: a float32 (h, w) or (h, w, 3) image")
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else 3
    if a.ndim == 3 and a.strides[2] != 4:
        a = np.ascontiguousarray(a)
    stride = a.strides[1] // 4
    if a.strides[1] % 4 or stride < ch or a.strides[0] != w * a.strides[1]:
        a = np.ascontiguousarray(a)
        stride = ch
    need = lib().rt3_frame_pfm_bytes(a.ctypes.data_as(C.c_void_p), w, h, ch, stride, None, 0)
    buf = np.zeros(need, np.uint8)
    got = lib().rt3_frame_pfm_bytes(a.ctypes.data_as(C.c_void_p), w, h, ch, stride, _p(buf), need)
    if need == 0 or got != need:
        raise ValueError("pfm_bytes: bad image")
    return buf.tobytes()


class Camera:
    """Pinhole camera owning a Frame; four public vectors as in Camera.hpp:27-34."""

    def __init__(self):
        self.c = rt3_camera()
        self.frame = None

    def update(self, width, height, focal_length, viewport_width, viewport_height):
        """Camera::update (Camera.cpp:77-96): origin 0, axis-aligned viewport, new Frame(width, height)."""
        self.frame = Frame(width, height)
        lib().rt3_camera_update(C.byref(self.c), np.float32(focal_length), np.float32(viewport_width),
                                np.float32(viewport_height))
        return self

    def look_at(self, width, height, look_from, look_at, vup=(0.0, 1.0, 0.0), vfov=20.0, focus_dist=1.0):
        """Extension: the book's look-from/look-at camera in the reference's four vectors."""
        self.frame = Frame(width, height)
        aspect = np.float32(np.float32(width) / np.float32(height))
        lib().rt3_camera_look_at(C.byref(self.c), _f3(look_from), _f3(look_at), _f3(vup), np.float32(vfov), aspect,
                                 np.float32(focus_dist))
        return self

    @property
    def origin(self):
        return tuple(self.c.origin)

    @property
    def horizontal(self):
        return tuple(self.c.horizontal)

    @property
    def vertical(self):
        return tuple(self.c.vertical)

    @property
    def lower_left_corner(self):
        return tuple(self.c.lower_left_corner)

    def w(self):
        return self.frame.w()

    def h(self):
        return self.frame.h()

    def get_frame(self):
        return self.frame


def main_camera(width, height):
    """The camera Main.cpp:272 builds: update(W, H, 2.0, (float(W)/float(H))*2.0f, 2.0f)."""
    vw = np.float32(np.float32(width) / np.float32(height)) * np.float32(2.0)
    return Camera().update(width, height, 2.0, vw, 2.0)


# --------------------------------------------------------------------------------------------------------
# Entities  (src/lib/entities/*.hpp) — plain records; pre-rendering happens in HipRenderer.prerender
# --------------------------------------------------------------------------------------------------------
et_none, et_triangle, et_sphere, et_object, et_analytic_sphere = 0, 1, 2, 3, 4
eprmf_none, eprmf_cpu, eprmf_gpu = 0, 1, 2
epro_none, epro_generate_triangle, epro_generate_sphere, epro_load_object_file = 0, 1, 2, 3


class RenderEntity:
    """RenderEntity.hpp:76-89."""
    type = et_none
    pre_render_mode = eprmf_cpu
    pre_render_operation = epro_none
    pre_render_faces = 0
    pre_render_vertices = 0
    material = None          # extension: rt3 material (kind, rgb, param); None = the reference's flat colour


def _material(kind, rgb, param=0.0):
    m = np.zeros(1, MATERIAL)
    m["rgb"][0] = rgb
    m["param"][0] = param
    m["kind"][0] = kind
    return m


def create_triangle(p1, p2, p3, color, material=None):
    """ECS::create_triangle (Triangle.cpp:28-53)."""
    e = RenderEntity()
    e.type, e.pre_render_operation = et_triangle, epro_generate_triangle
    e.pre_render_faces, e.pre_render_vertices = 1, 3
    e.points, e.color, e.material = (tuple(p1), tuple(p2), tuple(p3)), tuple(color), material
    return e


def create_sphere(center, radius, n_meridians, n_parallels, color, material=None):
    """ECS::create_sphere (Sphere.cpp:87-115).  Extension: n_meridians == n_parallels == 0 asks for an analytic
    sphere (Mode X) instead of a tessellation."""
    e = RenderEntity()
    e.center, e.radius, e.color, e.material = tuple(center), float(radius), tuple(color), material
    e.n_meridians, e.n_parallels = int(n_meridians), int(n_parallels)
    if n_meridians == 0 and n_parallels == 0:
        e.type = et_analytic_sphere
        return e
    e.type, e.pre_render_operation = et_sphere, epro_generate_sphere
    e.pre_render_mode = eprmf_cpu | eprmf_gpu          # Sphere.cpp:94-98: spheres can also be tessellated on the GPU
    e.pre_render_faces = lib().rt3_sphere_face_count(n_meridians, n_parallels)
    e.pre_render_vertices = lib().rt3_sphere_vertex_count(n_meridians, n_parallels)
    return e


def create_object(file_path, center, scale, color, material=None):
    """ECS::create_object (Object.cpp:54-126): opens the file once to count faces and vertices."""
    e = RenderEntity()
    e.type, e.pre_render_operation = et_object, epro_load_object_file
    e.file_path, e.center, e.scale, e.color, e.material = file_path, tuple(center), np.float32(scale), tuple(color), material
    nf, nv = C.c_uint32(), C.c_uint32()
    rc = lib().rt3_object_count(os.fsencode(file_path), C.byref(nf), C.byref(nv))
    if rc != 0:
        raise Fatal("Could not open file or unreadable line: %s" % file_path)
    e.pre_render_faces, e.pre_render_vertices = nf.value, nv.value
    return e


def lambertian(rgb):
    return _material(MAT_LAMBERT, rgb)


def metal(rgb, fuzz):
    return _material(MAT_METAL, rgb, fuzz)


def dielectric(ior):
    return _material(MAT_DIELECTRIC, (1.0, 1.0, 1.0), ior)


def emissive(rgb):
    return _material(MAT_FLAT, rgb)


def pre_render_entity(e):
    """cpu_pre_render_{triangle,sphere,object}: entity -> (GFace[], vec4[])."""
    faces = np.zeros(e.pre_render_faces, GFACE)
    verts = np.zeros((e.pre_render_vertices, 4), np.float32)
    if e.pre_render_operation == epro_generate_triangle:
        lib().rt3_prerender_triangle(_f3(e.points[0]), _f3(e.points[1]), _f3(e.points[2]), _f3(e.color), _p(faces), _p(verts))
    elif e.pre_render_operation == epro_generate_sphere:
        lib().rt3_prerender_sphere(_f3(e.center), np.float32(e.radius), e.n_meridians, e.n_parallels, _f3(e.color),
                                   _p(faces), _p(verts))
    elif e.pre_render_operation == epro_load_object_file:
        rc = lib().rt3_prerender_object(os.fsencode(e.file_path), _f3(e.center), e.scale, _f3(e.color), _p(faces),
                                        len(faces), _p(verts), len(verts))
        if rc != 0:
            raise Fatal("Could not load object file '%s'" % e.file_path)
    else:
        raise Fatal("Entity wants to be pre-rendered using unsupported operation %d" % e.pre_render_operation)
    return faces, verts


def merge_entities(parts):
    """SequentialRenderer::transfer_entity over a list of (faces, verts): indices rebased by running vertex count."""
    nf = sum(len(f) for f, _ in parts)
    nv = sum(len(v) for _, v in parts)
    faces = np.zeros(nf, GFACE)
    verts = np.zeros((nv, 4), np.float32)
    cf, cv = C.c_uint32(0), C.c_uint32(0)
    for f, v in parts:
        f = np.ascontiguousarray(f)
        v = np.ascontiguousarray(v, np.float32)
        lib().rt3_transfer_entity(_p(faces), C.byref(cf), _p(verts), C.byref(cv), _p(f), len(f), _p(v), len(v))
    return faces, verts


# --------------------------------------------------------------------------------------------------------
# benchmark scenes
# --------------------------------------------------------------------------------------------------------
def _sphere_scene(fn, *args):
    n = fn(*args, None, None, 0)
    cr = np.zeros((n, 4), np.float32)
    mats = np.zeros(n, MATERIAL)
    got = fn(*args, _p(cr), _p(mats), n)
    assert got == n
    return cr, mats


def scene_three_spheres():
    return _sphere_scene(lib().rt3_scene_three_spheres)


def scene_weekend(seed=42):
    return _sphere_scene(lib().rt3_scene_weekend, seed)


def scene_stress(n=100000, seed=43):
    return _sphere_scene(lib().rt3_scene_stress, n, seed)


def scene_cornell(grid=64):
    n = lib().rt3_scene_cornell(grid, None, None, None, 0)
    faces = np.zeros(n, GFACE)
    verts = np.zeros((3 * n, 4), np.float32)
    mats = np.zeros(n, MATERIAL)
    got = lib().rt3_scene_cornell(grid, _p(faces), _p(verts), _p(mats), n)
    assert got == n
    return faces, verts, mats


def weekend_camera(width, height):
    """Book final-scene camera: from (13,2,3) at (0,0,0), vfov 20, focus distance 10."""
    return Camera().look_at(width, height, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 10.0)


def make_params(width, height, spp=1, max_depth=1, seed=1, flags=0, lens_radius=0.0, t_min=0.001,
                tile_rows=8, tile_index=0, tile_count=1):
    return rt3_params(width, height, spp, max_depth, seed, flags, lens_radius, t_min, tile_rows, tile_index, tile_count)


# --------------------------------------------------------------------------------------------------------
# Renderer  (src/lib/renderer/Renderer.hpp:34-63)
# --------------------------------------------------------------------------------------------------------
class Renderer:
    """Abstract backend API of the reference."""

    def prerender(self, entities):
        raise NotImplementedError

    def render(self, camera):
        raise NotImplementedError


class HipRenderer(Renderer):
    """The MI355X backend.  Mode R by default; ``configure(spp=..., max_depth=...)`` switches render() to Mode X."""

    def __init__(self, device=0):
        self._ctx = lib().rt3_create(device)
        if not self._ctx:
            raise Fatal(lib().rt3_last_error(None).decode())
        self._path = None            # rt3_params template when Mode X is requested
        self.n_faces = 0
        self.n_spheres = 0
        self._mesh_counts = (0, 0)
        self._torch_device = None    # set by a device-form upload or update: regroup() then queues on torch's current stream as well

    def close(self):
        if getattr(self, "_ctx", None):
            lib().rt3_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise Fatal(lib().rt3_last_error(self._ctx).decode())

    # -- scene ---------------------------------------------------------------------------------------
    def prerender(self, entities, gpu_prerender=False):
        """Renderer::prerender: flatten the entities (order = array order) into the device buffers.  Replaces the old
        scene.  With gpu_prerender, entities flagged eprmf_gpu (tessellated spheres, as in the reference's Vulkan build)
        are generated on the device at their running offsets (VulkanRenderer.cpp:305-327); everything else is
        pre-rendered on the host and transferred (VulkanRenderer.cpp:355-387)."""
        mesh_ents, spheres, smats = [], [], []
        for i, e in enumerate(entities):
            if e.type == et_analytic_sphere:
                spheres.append((e.center[0], e.center[1], e.center[2], e.radius))
                smats.append(e.material if e.material is not None else _material(MAT_FLAT, e.color))
            elif not (e.pre_render_mode & (eprmf_cpu | eprmf_gpu)):
                raise Fatal("Entity %d cannot be pre-rendered by this back-end." % i)
            else:
                mesh_ents.append(e)
        nf = sum(e.pre_render_faces for e in mesh_ents)
        nv = sum(e.pre_render_vertices for e in mesh_ents)
        any_mat = any(e.material is not None for e in mesh_ents)
        self._check(lib().rt3_mesh_begin(self._ctx, nf, nv))
        fo = vo = 0
        part_mats = []
        for e in mesh_ents:
            if gpu_prerender and (e.pre_render_mode & eprmf_gpu) and e.pre_render_operation == epro_generate_sphere:
                self._check(lib().rt3_mesh_sphere(self._ctx, _f3(e.center), np.float32(e.radius), e.n_meridians, e.n_parallels,
                                                  _f3(e.color), fo, vo))
                colors = None
            else:
                f, v = pre_render_entity(e)
                self._check(lib().rt3_mesh_put(self._ctx, _p(f), len(f), _p(v), len(v), fo, vo))
                colors = f["color"]
            if any_mat:
                if e.material is not None:
                    part_mats.append(np.repeat(e.material, e.pre_render_faces))
                else:
                    if colors is None:
                        raise Fatal("a device-tessellated sphere needs a material when other entities have one")
                    m = np.zeros(e.pre_render_faces, MATERIAL)
                    m["rgb"] = colors
                    m["kind"] = MAT_FLAT
                    part_mats.append(m)
            fo += e.pre_render_faces
            vo += e.pre_render_vertices
        fmats = np.ascontiguousarray(np.concatenate(part_mats)) if (mesh_ents and any_mat) else None
        self._check(lib().rt3_mesh_commit(self._ctx, _p(fmats)))
        self.n_faces = nf
        self._mesh_counts = (nf, nv)
        if spheres:
            self.set_spheres(np.array(spheres, np.float32), np.concatenate(smats))
        else:
            self.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, MATERIAL))

    def mesh_download(self):
        """The merged GFace[] / vec4[] as they sit on the device (after prerender / set_mesh)."""
        nf, nv = getattr(self, "_mesh_counts", (0, 0))
        faces = np.zeros(nf, GFACE)
        verts = np.zeros((nv, 4), np.float32)
        self._check(lib().rt3_mesh_download(self._ctx, _p(faces), _p(verts)))
        return faces, verts

    def set_mesh(self, faces, verts, face_materials=None):
        """The merged mesh (rt3_set_mesh).  numpy arrays: the host upload, synchronous.  Contiguous torch GPU tensors on one device — verts
        float32 (n, 4), faces any tensor of n 48-byte records, face_materials None or n 20-byte records — are read in place and the scene is
        built on the device, queued on torch.cuda.current_stream() (rt3_set_mesh_device): the state of the host upload
        followed by regroup().  The call waits for the device once."""
        nv = self._torch_rows(verts, "verts", 16)
        if nv is not None:
            import torch
            if verts.dtype != torch.float32:
                raise Fatal("device verts must be float32")
            nf = self._torch_rows(faces, "faces", GFACE.itemsize)
            if nf is None or faces.device != verts.device:
                raise Fatal("device faces must be a GPU tensor on the verts' device")
            mptr = None
            if face_materials is not None:
                if self._torch_rows(face_materials, "face_materials", MATERIAL.itemsize) != nf or face_materials.device != verts.device:
                    raise Fatal("device face_materials must hold one 20-byte record per face, on the verts' device")
                mptr = C.c_void_p(face_materials.data_ptr())
            stream = torch.cuda.current_stream(verts.device).cuda_stream
            self._torch_device = verts.device
            self._check(lib().rt3_set_mesh_device(self._ctx, C.c_void_p(faces.data_ptr()) if nf else None, nf,
                                                  C.c_void_p(verts.data_ptr()) if nv else None, nv, mptr, C.c_void_p(stream)))
            self.n_faces = nf
            self._mesh_counts = (nf, nv)
            return
        faces = np.ascontiguousarray(faces)
        verts = np.ascontiguousarray(verts, np.float32)
        assert faces.dtype == GFACE
        if face_materials is not None:
            face_materials = np.ascontiguousarray(face_materials)
            assert face_materials.dtype == MATERIAL and len(face_materials) == len(faces)
        self._torch_device = None
        self._check(lib().rt3_set_mesh(self._ctx, _p(faces), len(faces), _p(verts), len(verts), _p(face_materials)))
        self.n_faces = len(faces)
        self._mesh_counts = (len(faces), len(verts))

    def set_spheres(self, center_radius, materials):
        """The analytic spheres (rt3_set_spheres).  numpy arrays: the host upload, synchronous.  Contiguous torch GPU tensors on one device —
        center_radius float32 (n, 4), materials any tensor of n 20-byte records — are read in place and the scene is built on the device,
        queued on torch.cuda.current_stream() (rt3_set_spheres_device): the state of the host upload followed by regroup().
        The call waits for the device once; a radius that is not > 0 or an unknown material kind is refused with the scene untouched."""
        n = self._torch_rows(center_radius, "center_radius", 16)
        if n is not None:
            import torch
            if center_radius.dtype != torch.float32:
                raise Fatal("device center_radius must be float32")
            if self._torch_rows(materials, "materials", MATERIAL.itemsize) != n or materials.device != center_radius.device:
                raise Fatal("device materials must hold one 20-byte record per sphere, on center_radius' device")
            stream = torch.cuda.current_stream(center_radius.device).cuda_stream
            self._torch_device = center_radius.device
            self._check(lib().rt3_set_spheres_device(self._ctx, C.c_void_p(center_radius.data_ptr()) if n else None,
                                                     C.c_void_p(materials.data_ptr()) if n else None, n, C.c_void_p(stream)))
            self.n_spheres = n
            return
        cr = np.ascontiguousarray(center_radius, np.float32).reshape(-1, 4)
        materials = np.ascontiguousarray(materials)
        assert materials.dtype == MATERIAL and len(materials) == len(cr)
        self._torch_device = None
        self._check(lib().rt3_set_spheres(self._ctx, _p(cr), _p(materials), len(cr)))
        self.n_spheres = len(cr)

    def sphere_build(self):
        """Tests: the filter centre (3 float32) and the direct list (sorted uint32) the context holds after the last sphere upload
        (rt3_debug_sphere_build)."""
        centre = np.zeros(3, np.float32)
        direct = np.zeros(4, np.uint32)
        n = C.c_uint32(0)
        self._check(lib().rt3_debug_sphere_build(self._ctx, _p(centre), _p(direct), C.byref(n)))
        return centre, np.sort(direct[:n.value])

    # -- refit: new positions for the scene that is there (rt3_update_*) -----------------------------
    @staticmethod
    def _torch_rows(t, what, row_bytes):
        """A torch tensor on the GPU holding rows of row_bytes bytes each -> its row count, or None for a host array."""
        if not type(t).__module__.startswith("torch"):
            return None
        if not t.is_cuda or not t.is_contiguous() or t.dim() < 1 or (t.numel() * t.element_size()) % row_bytes:
            raise Fatal("device %s must be a contiguous GPU tensor of %d-byte records" % (what, row_bytes))
        return t.numel() * t.element_size() // row_bytes

    def update_spheres(self, center_radius):
        """New (cx, cy, cz, r) for every sphere of the scene (rt3_update_spheres): the result of set_spheres(center_radius, <the same
        materials>) without the host-side rebuild; the grouping of the last set_spheres is kept.  numpy (n, 4): synchronous.  A contiguous
        (n, 4) float32 torch tensor on the GPU is read in place, queued on torch.cuda.current_stream() (rt3_update_spheres_device)."""
        n = self._torch_rows(center_radius, "center_radius", 16)
        if n is not None:
            import torch
            if center_radius.dtype != torch.float32:
                raise Fatal("device center_radius must be float32")
            stream = torch.cuda.current_stream(center_radius.device).cuda_stream
            self._torch_device = center_radius.device
            self._check(lib().rt3_update_spheres_device(self._ctx, C.c_void_p(center_radius.data_ptr()), n, C.c_void_p(stream)))
            return
        cr = np.ascontiguousarray(center_radius, np.float32).reshape(-1, 4)
        self._torch_device = None
        self._check(lib().rt3_update_spheres(self._ctx, _p(cr), len(cr)))

    def update_mesh(self, vertices, faces=None):
        """New merged vertices ((n_vertices, 4), as mesh_download returns them) for the committed mesh (rt3_update_mesh); faces None keeps
        the indices, stored normals and colours, a GFACE array of the mesh's face count replaces them (new normals).  numpy: synchronous.
        torch: contiguous GPU tensors (vertices float32 (n, 4); faces any tensor of n_faces 48-byte records), read in place and queued on
        torch.cuda.current_stream() (rt3_update_mesh_device)."""
        n = self._torch_rows(vertices, "vertices", 16)
        if n is not None:
            import torch
            if vertices.dtype != torch.float32:
                raise Fatal("device vertices must be float32")
            fptr = None
            if faces is not None:
                if self._torch_rows(faces, "faces", GFACE.itemsize) != self.n_faces or faces.device != vertices.device:
                    raise Fatal("device faces must hold the mesh's %d faces, on the vertices' device" % self.n_faces)
                fptr = C.c_void_p(faces.data_ptr())
            stream = torch.cuda.current_stream(vertices.device).cuda_stream
            self._torch_device = vertices.device
            self._check(lib().rt3_update_mesh_device(self._ctx, fptr, C.c_void_p(vertices.data_ptr()), n, C.c_void_p(stream)))
            return
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        self._torch_device = None
        f = None
        if faces is not None:
            f = np.ascontiguousarray(faces)
            if f.dtype != GFACE or len(f) != self.n_faces:
                raise Fatal("update_mesh: faces must be a GFACE array of the mesh's %d faces" % self.n_faces)
        self._check(lib().rt3_update_mesh(self._ctx, _p(f), _p(v), len(v)))

    def regroup(self, spheres=True, mesh=True):
        """The group order of the candidate filter again, from the positions on the device (rt3_regroup): what repeated
        updates let go stale, without a full upload.  Results do not change, only the filter's work.  Regroups the named classes that
        have a committed scene.  Synchronous, unless the last upload or update of the scene was an update from torch tensors: then
        it is queued on torch.cuda.current_stream() like that update (rt3_regroup_device)."""
        what = (REGROUP_SPHERES if spheres and self.n_spheres else 0) | (REGROUP_MESH if mesh and self.n_faces else 0)
        if not what:
            return
        if self._torch_device is not None:
            import torch
            stream = torch.cuda.current_stream(self._torch_device).cuda_stream
            self._check(lib().rt3_regroup_device(self._ctx, what, C.c_void_p(stream)))
            return
        self._check(lib().rt3_regroup(self._ctx, what))

    def group_order(self, what):
        """Tests: the group order of one class (REGROUP_SPHERES or REGROUP_MESH) as rt3_debug_group_order downloads it: the primitive
        index at every position, 0xFFFFFFFF for a pad."""
        n = C.c_uint32(0)
        rc = lib().rt3_debug_group_order(self._ctx, what, None, 0, C.byref(n))
        if rc != 0 and n.value == 0:
            self._check(rc)
        out = np.zeros(n.value, np.uint32)
        self._check(lib().rt3_debug_group_order(self._ctx, what, _p(out), len(out), C.byref(n)))
        return out

    def synchronize(self):
        """rt3_synchronize: waits for the context's own stream; reports a face index out of range of a device-form update_mesh."""
        self._check(lib().rt3_synchronize(self._ctx))

    # -- render --------------------------------------------------------------------------------------
    def configure(self, spp=None, max_depth=None, seed=1, flags=0, lens_radius=0.0, t_min=0.001):
        """spp=None returns render() to Mode R."""
        self._path = None if spp is None else dict(spp=spp, max_depth=max_depth or 1, seed=seed, flags=flags,
                                                   lens_radius=lens_radius, t_min=t_min)

    def render(self, camera):
        """Renderer::render: writes the pixels into camera.get_frame().d()."""
        frame = camera.get_frame()
        if self._path is None:
            self._check(lib().rt3_render(self._ctx, C.byref(camera.c), frame.w(), frame.h(), _p(frame.data)))
        else:
            p = make_params(frame.w(), frame.h(), **self._path)
            self._check(lib().rt3_render_path(self._ctx, C.byref(camera.c), C.byref(p), _p(frame.data)))

    def render_path(self, camera_c, params):
        """Mode X with explicit params (tiles included); returns the compact (rows_owned, width) pixel array."""
        rows = lib().rt3_rows_owned(C.byref(params))
        out = np.zeros((rows, params.width), np.uint32)
        self._check(lib().rt3_render_path(self._ctx, C.byref(camera_c), C.byref(params), _p(out)))
        return out

    def render_path_range(self, camera_c, params, sample_begin, sample_count):
        """Progressive Mode X (rt3_render_path_range): adds samples [begin, begin + count) to the accumulation this renderer
        keeps and returns the frame resolved over the samples so far.  begin == 0 starts over."""
        rows = lib().rt3_rows_owned(C.byref(params))
        out = np.zeros((rows, params.width), np.uint32)
        self._check(lib().rt3_render_path_range(self._ctx, C.byref(camera_c), C.byref(params), sample_begin, sample_count, _p(out)))
        return out

    def render_path_range_device(self, camera_c, params, sample_begin, sample_count, d_out_ptr, stream_ptr=None):
        self._check(lib().rt3_render_path_range_device(self._ctx, C.byref(camera_c), C.byref(params), sample_begin, sample_count,
                                                       C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    # -- adaptive sampling (rt3_render_path_adaptive*) ------------------------------------------------
    def render_adaptive(self, camera_c, params, threshold=0.05, min_spp=16, step_spp=16, dark=0.01):
        """Mode X with params.spp as a budget: min_spp samples for every pixel, then step_spp at a time for the pixels whose 3 x 3
        neighbourhood has not reached a relative standard error of `threshold`.  Returns (pixels, counts), both uint32 (rows_owned, width):
        a pixel with count n is the pixel of render_path_range(camera_c, params, 0, n), bit for bit.  accum_resolve() afterwards gives the
        linear frame (each pixel over its own count) for the denoiser."""
        rows = lib().rt3_rows_owned(C.byref(params))
        out = np.zeros((rows, params.width), np.uint32)
        counts = np.zeros((rows, params.width), np.uint32)
        ap = ADAPTIVE_PARAMS(min_spp, step_spp, threshold, dark)
        self._check(lib().rt3_render_path_adaptive(self._ctx, C.byref(camera_c), C.byref(params), C.byref(ap), _p(out), _p(counts)))
        return out, counts

    def render_adaptive_device(self, camera_c, params, d_out, d_counts=None, stream_ptr=None, threshold=0.05, min_spp=16, step_spp=16, dark=0.01):
        """The same into device memory (rt3_render_path_adaptive_device).  d_out / d_counts: raw device pointers (ints; the work is queued
        on stream_ptr, None = the renderer's own stream) or contiguous 4-byte torch tensors of rows_owned * width elements on the GPU (queued
        on torch.cuda.current_stream() unless stream_ptr is given); d_counts may be None.  The call waits for the device once per round."""
        n = lib().rt3_rows_owned(C.byref(params)) * params.width
        ptrs = []
        for t, what in ((d_out, "d_out"), (d_counts, "d_counts")):
            if t is not None and type(t).__module__.startswith("torch"):
                if self._torch_rows(t, what, 4) != n:
                    raise Fatal("device %s must hold rows_owned * width = %d 4-byte elements" % (what, n))
                if stream_ptr is None:
                    import torch
                    stream_ptr = torch.cuda.current_stream(t.device).cuda_stream
                t = t.data_ptr()
            ptrs.append(C.c_void_p(t or 0))
        ap = ADAPTIVE_PARAMS(min_spp, step_spp, threshold, dark)
        self._check(lib().rt3_render_path_adaptive_device(self._ctx, C.byref(camera_c), C.byref(params), C.byref(ap), ptrs[0], ptrs[1],
                                                          C.c_void_p(stream_ptr or 0)))

    def accum_download(self, params, want_sq=False):
        """Checkpoint of the accumulation: (sum[rows, w, 4], sum_sq or None, samples_done)."""
        rows = lib().rt3_rows_owned(C.byref(params))
        acc = np.zeros((rows, params.width, 4), np.float32)
        sq = np.zeros((rows, params.width, 4), np.float32) if want_sq else None
        done = C.c_uint32(0)
        self._check(lib().rt3_accum_download(self._ctx, _p(acc), _p(sq), C.byref(done)))
        return acc, sq, done.value

    def accum_upload(self, camera_c, params, acc, sq, samples_done):
        acc = np.ascontiguousarray(acc, np.float32)
        sq = None if sq is None else np.ascontiguousarray(sq, np.float32)
        self._check(lib().rt3_accum_upload(self._ctx, C.byref(camera_c), C.byref(params), _p(acc), _p(sq), samples_done))

    def gather_rows(self, d_frame_ptr, shard_renderer, d_tile_ptr, shard_params, stream_ptr=None):
        """rt3_gather_rows: the shard's compact rows -> their interleaved places in this (root) renderer's device frame."""
        self._check(lib().rt3_gather_rows(self._ctx, C.c_void_p(d_frame_ptr), shard_renderer._ctx, C.c_void_p(d_tile_ptr),
                                          C.byref(shard_params), C.c_void_p(stream_ptr or 0)))

    def force_brute(self, on):
        """Tests / fuzzers: the unfiltered Mode-X kernel (every ray against every primitive)."""
        self._check(lib().rt3_debug_force_brute(self._ctx, 1 if on else 0))

    def force_flat_filter(self, on):
        """Tests / A-B: the tiled matrix-filter kernel with one row per primitive instead of the two-level filter's group rows (same pixels)."""
        self._check(lib().rt3_debug_force_flat_filter(self._ctx, 1 if on else 0))

    def render_path_device(self, camera_c, params, d_out_ptr, stream_ptr=None):
        """Asynchronous Mode X into a device buffer (e.g. a torch tensor's data_ptr()) on a HIP stream."""
        self._check(lib().rt3_render_path_device(self._ctx, C.byref(camera_c), C.byref(params), C.c_void_p(d_out_ptr),
                                                 C.c_void_p(stream_ptr or 0)))

    def render_device(self, camera_c, width, height, d_out_ptr, stream_ptr=None):
        self._check(lib().rt3_render_device(self._ctx, C.byref(camera_c), width, height, C.c_void_p(d_out_ptr),
                                            C.c_void_p(stream_ptr or 0)))

    # -- batched ray queries (rt3_intersect* / rt3_occluded*) ------------------------------------
    @staticmethod
    def _torch_rays(rays):
        """A torch tensor of rays on the GPU, or None for host rays."""
        mod = type(rays).__module__
        if not mod.startswith("torch"):
            return None
        if not rays.is_cuda or str(rays.dtype) != "torch.float32" or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise Fatal("device rays must be a contiguous (N, 8) float32 tensor on the GPU")
        return rays

    @staticmethod
    def _host_rays(rays):
        a = np.asarray(rays)
        if a.dtype == RAY:
            return np.ascontiguousarray(a).reshape(-1)
        if a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 8:
            return np.ascontiguousarray(a).view(RAY).reshape(-1)
        raise Fatal("rays must be a RAY array or an (N, 8) float32 array")

    def _query(self, rays, t_min, occluded):
        t = self._torch_rays(rays)
        if t is not None:
            import torch
            n = t.shape[0]
            out = torch.empty((n,) if occluded else (n, 4), dtype=torch.int32, device=t.device)
            stream = torch.cuda.current_stream(t.device).cuda_stream
            fn = lib().rt3_occluded_device if occluded else lib().rt3_intersect_device
            self._check(fn(self._ctx, C.c_void_p(t.data_ptr()), n, np.float32(t_min), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
            if occluded:
                return out
            return out[:, 0].view(torch.float32), out[:, 1], out[:, 2]
        r = self._host_rays(rays)
        out = np.zeros(len(r), np.uint32 if occluded else HIT)
        fn = lib().rt3_occluded if occluded else lib().rt3_intersect
        self._check(fn(self._ctx, _p(r), len(r), np.float32(t_min), _p(out)))
        return out

    def intersect(self, rays, t_min=0.001):
        """Nearest hit of every ray (rt3_intersect).  numpy RAY / (N, 8) float32 -> numpy HIT array; a contiguous (N, 8) float32 torch
        tensor on the GPU -> (t, kind, index), views of one (N, 4) int32 tensor, computed on torch.cuda.current_stream()."""
        return self._query(rays, t_min, False)

    def occluded(self, rays, t_min=0.001):
        """1 where a ray hits something before its t_max, 0 where not, 0xFFFFFFFF for an invalid ray (rt3_occluded): numpy uint32 for host
        rays, an (N,) int32 tensor for device rays."""
        return self._query(rays, t_min, True)

    # -- radiance along caller-supplied rays (rt3_radiance*) -----------------------------------------
    def radiance(self, rays, keys=None, samples=1, sample_begin=0, max_depth=8, seed=1, flags=0, t_min=0.001):
        """Path-traced radiance along every ray (rt3_radiance): the mean over samples [sample_begin, sample_begin + samples) of the Mode-X
        path that starts with the ray (flags: FLAG_BLACK_BACKGROUND, FLAG_ENV_SAMPLING or FLAG_LIGHT_SAMPLING, the last two not together), keyed by keys[i] (default: the ray's index) where a render keys by the pixel index.  numpy RAY /
        (N, 8) float32 (keys: (N,) uint32) -> float32 (N, 4), (r, g, b, 0), NaN rgb for an invalid ray; a contiguous (N, 8) float32 torch
        tensor on the GPU (keys: an (N,) int32 tensor on that device) -> an (N, 4) float32 tensor there, computed on
        torch.cuda.current_stream()."""
        rp = RADIANCE_PARAMS(max_depth, seed, flags, sample_begin, samples, np.float32(t_min))
        t = self._torch_rays(rays)
        if t is not None:
            import torch
            n = t.shape[0]
            if keys is not None and (not type(keys).__module__.startswith("torch") or keys.device != t.device or keys.dtype != torch.int32 or
                                     keys.dim() != 1 or keys.shape[0] != n or not keys.is_contiguous()):
                raise Fatal("device keys must be a contiguous (N,) int32 tensor on the rays' device")
            out = torch.empty((n, 4), dtype=torch.float32, device=t.device)
            stream = torch.cuda.current_stream(t.device).cuda_stream
            self.radiance_device(t.data_ptr(), None if keys is None else keys.data_ptr(), n, rp, out.data_ptr(), stream)
            return out
        r = self._host_rays(rays)
        k = None
        if keys is not None:
            k = np.ascontiguousarray(keys, np.uint32).reshape(-1)
            if len(k) != len(r):
                raise Fatal("keys and rays differ in length")
        out = np.zeros((len(r), 4), np.float32)
        self._check(lib().rt3_radiance(self._ctx, _p(r), _p(k), len(r), C.byref(rp), _p(out)))
        return out

    def radiance_device(self, d_rays_ptr, d_keys_ptr, n, radiance_params, d_out_ptr, stream_ptr=None):
        """Asynchronous rt3_radiance_device: n rt3_ray at d_rays_ptr, n uint32 keys at d_keys_ptr (or None), n float4 out at d_out_ptr."""
        self._check(lib().rt3_radiance_device(self._ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_keys_ptr or 0), n, C.byref(radiance_params),
                                              C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    # -- lens models (rt3_lens_rays*, rt3_render_lens*, rt3_render_lens_aov*) ------------------------------------------
    @staticmethod
    def _lens_range(params, sample_begin, sample_count):
        return int(sample_begin), int(params.spp - sample_begin if sample_count is None else sample_count)

    def lens_rays(self, lens, params, sample_begin=0, sample_count=None, device=None):
        """The lens's rays for samples [begin, begin + count) (default: all spp), sample-major as camera_rays returns the camera's: a RAY array,
        or with device (a torch device, or True for the current one) a (n, 8) float32 tensor there, queued on torch.cuda.current_stream()."""
        sb, sc = self._lens_range(params, sample_begin, sample_count)
        n = lib().rt3_rows_owned(C.byref(params)) * params.width * max(sc, 0)
        if device is not None and device is not False:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device()) if device is True else torch.device(device)
            out = torch.empty((n, 8), dtype=torch.float32, device=dev)
            self.lens_rays_device(lens, params, sb, sc, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out
        out = np.zeros(n, RAY)
        self._check(lib().rt3_lens_rays(self._ctx, C.byref(lens), C.byref(params), sb, sc, _p(out)))
        return out

    def lens_rays_device(self, lens, params, sample_begin, sample_count, d_out_ptr, stream_ptr=None):
        self._check(lib().rt3_lens_rays_device(self._ctx, C.byref(lens), C.byref(params), sample_begin, sample_count, C.c_void_p(d_out_ptr),
                                               C.c_void_p(stream_ptr or 0)))

    def render_lens(self, lens, params, sample_begin=0, sample_count=None, device=None):
        """The lens frame, linear (rt3_render_lens): the mean radiance over samples [begin, begin + count) (default: all spp) of every owned pixel,
        float32 (rows_owned, width, 4), (r, g, b, 0) — a numpy array, or with device (a torch device, or True for the current one) a tensor there,
        queued on torch.cuda.current_stream().  A cube lens's frame, reshaped to (6, N, N, 4), is what set_environment takes."""
        sb, sc = self._lens_range(params, sample_begin, sample_count)
        rows = lib().rt3_rows_owned(C.byref(params))
        if device is not None and device is not False:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device()) if device is True else torch.device(device)
            out = torch.empty((rows, params.width, 4), dtype=torch.float32, device=dev)
            self.render_lens_device(lens, params, sb, sc, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out
        out = np.zeros((rows, params.width, 4), np.float32)
        self._check(lib().rt3_render_lens(self._ctx, C.byref(lens), C.byref(params), sb, sc, _p(out)))
        return out

    def render_lens_device(self, lens, params, sample_begin, sample_count, d_out_ptr, stream_ptr=None):
        """Asynchronous rt3_render_lens_device into a device buffer of rows_owned * width float4."""
        self._check(lib().rt3_render_lens_device(self._ctx, C.byref(lens), C.byref(params), sample_begin, sample_count, C.c_void_p(d_out_ptr),
                                                 C.c_void_p(stream_ptr or 0)))

    def render_lens_aov(self, lens, params, device=None):
        """First-hit AOVs of the lens frame (rt3_render_lens_aov): an AOV array of shape (rows_owned, width), or with device a (rows_owned, width,
        12) float32 tensor of the 48-byte records there, queued on torch.cuda.current_stream() — what denoise() takes beside render_lens()."""
        rows = lib().rt3_rows_owned(C.byref(params))
        if device is not None and device is not False:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device()) if device is True else torch.device(device)
            out = torch.empty((rows, params.width, 12), dtype=torch.float32, device=dev)
            self.render_lens_aov_device(lens, params, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out
        out = np.zeros((rows, params.width), AOV)
        self._check(lib().rt3_render_lens_aov(self._ctx, C.byref(lens), C.byref(params), _p(out)))
        return out

    def render_lens_aov_device(self, lens, params, d_out_ptr, stream_ptr=None):
        self._check(lib().rt3_render_lens_aov_device(self._ctx, C.byref(lens), C.byref(params), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    def render_lens_aov_specular(self, lens, params, max_bounces=8, max_fuzz=0.0, device=None):
        """Specular-chain AOVs of the lens frame (rt3_render_lens_aov_specular): render_lens_aov with every ray followed through
        glass and metals of fuzz <= max_fuzz; numpy, or with device a (rows_owned, width, 12) float32 tensor there, as render_lens_aov."""
        rows = lib().rt3_rows_owned(C.byref(params))
        chain = rt3_aov_chain_params(max_bounces, max_fuzz, 0, 0)
        if device is not None and device is not False:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device()) if device is True else torch.device(device)
            out = torch.empty((rows, params.width, 12), dtype=torch.float32, device=dev)
            self._check(lib().rt3_render_lens_aov_specular_device(self._ctx, C.byref(lens), C.byref(params), C.byref(chain),
                                                                  C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            return out
        out = np.zeros((rows, params.width), AOV)
        self._check(lib().rt3_render_lens_aov_specular(self._ctx, C.byref(lens), C.byref(params), C.byref(chain), _p(out)))
        return out

    # -- image textures (rt3_set_texture*, rt3_bind_*_textures*) ---------------------------------------
    def set_texture(self, slot, image, wrap="repeat"):
        """Fills texture slot `slot` (< TEX_MAX_TEXTURES) with a copy of `image`: a numpy array (H, W, 3 | 4), row 0 on top, or a contiguous
        (H, W, 4) float32 torch tensor on the GPU, copied on torch.cuda.current_stream() (rt3_set_texture_device; its texels are not validated).
        wrap: "repeat" or "clamp", for both axes.  None frees the slot."""
        if image is None:
            self._check(lib().rt3_set_texture(self._ctx, int(slot), None, 0, 0, 0))
            return
        if type(image).__module__.startswith("torch"):
            import torch
            if not image.is_cuda or image.dtype != torch.float32 or image.dim() != 3 or image.shape[2] != 4 or not image.is_contiguous():
                raise Fatal("a device texture must be a contiguous (H, W, 4) float32 tensor on the GPU")
            stream = torch.cuda.current_stream(image.device).cuda_stream
            self._check(lib().rt3_set_texture_device(self._ctx, int(slot), C.c_void_p(image.data_ptr()), int(image.shape[1]), int(image.shape[0]),
                                                     _tex_wrap(wrap), C.c_void_p(stream or 0)))
            return
        rgba = _image_rgba(image)
        self._check(lib().rt3_set_texture(self._ctx, int(slot), _p(rgba), rgba.shape[1], rgba.shape[0], _tex_wrap(wrap)))

    def clear_textures(self):
        """Empties every slot and drops both bindings (rt3_clear_textures)."""
        self._check(lib().rt3_clear_textures(self._ctx))

    def texture_size(self, slot):
        """(W, H, wrap) of the texture in `slot`, wrap as "repeat" or "clamp"; (0, 0, "repeat") for an empty slot (rt3_texture_size)."""
        w, h, wrap = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(lib().rt3_texture_size(self._ctx, int(slot), C.byref(w), C.byref(h), C.byref(wrap)))
        return int(w.value), int(h.value), "clamp" if wrap.value == TEX_CLAMP else "repeat"

    def bind_sphere_textures(self, slots):
        """One texture slot per sphere, in the order of set_spheres (TEX_NONE: untextured); None unbinds the spheres.  numpy / a sequence, or a
        contiguous int32 / uint32 torch tensor on the GPU, read on torch.cuda.current_stream() (rt3_bind_sphere_textures_device).  The binding
        survives update_spheres() and regroup(); set_spheres() drops it."""
        if slots is None:
            self._check(lib().rt3_bind_sphere_textures(self._ctx, None, 0))
            return
        if type(slots).__module__.startswith("torch"):
            import torch
            if not slots.is_cuda or slots.dtype not in _torch_word_dtypes() or slots.dim() != 1 or not slots.is_contiguous():
                raise Fatal("device texture slots must be a contiguous 1-D int32 / uint32 tensor on the GPU")
            stream = torch.cuda.current_stream(slots.device).cuda_stream
            self._check(lib().rt3_bind_sphere_textures_device(self._ctx, C.c_void_p(slots.data_ptr()), int(slots.shape[0]), C.c_void_p(stream or 0)))
            return
        s = np.ascontiguousarray(np.asarray(slots, np.int64).astype(np.uint32).reshape(-1))
        self._check(lib().rt3_bind_sphere_textures(self._ctx, _p(s), len(s)))

    def bind_mesh_textures(self, slots, uv):
        """One texture slot per committed face (TEX_NONE: untextured) and the faces' texture coordinates, uv (n_faces, 3, 2) or (n_faces, 6):
        (u, v) of the face's first, second and third vertex; slots None unbinds the mesh.  numpy, or contiguous torch tensors on the GPU (slots
        int32 / uint32, uv float32), read on torch.cuda.current_stream() (rt3_bind_mesh_textures_device; uv is not validated).  The binding survives
        update_mesh() and regroup(); a new mesh drops it."""
        if slots is None:
            self._check(lib().rt3_bind_mesh_textures(self._ctx, None, None, 0))
            return
        if type(slots).__module__.startswith("torch"):
            import torch
            if (not slots.is_cuda or slots.dtype not in _torch_word_dtypes() or slots.dim() != 1 or not slots.is_contiguous() or
                    not type(uv).__module__.startswith("torch") or not uv.is_cuda or uv.dtype != torch.float32 or not uv.is_contiguous() or
                    uv.numel() != 6 * slots.shape[0]):
                raise Fatal("device texture slots must be a contiguous 1-D int32 / uint32 tensor and uv a contiguous float32 tensor of 6 floats per face, both on the GPU")
            stream = torch.cuda.current_stream(slots.device).cuda_stream
            self._check(lib().rt3_bind_mesh_textures_device(self._ctx, C.c_void_p(slots.data_ptr()), C.c_void_p(uv.data_ptr()), int(slots.shape[0]),
                                                            C.c_void_p(stream or 0)))
            return
        s = np.ascontiguousarray(np.asarray(slots, np.int64).astype(np.uint32).reshape(-1))
        t = np.ascontiguousarray(np.asarray(uv, np.float32).reshape(-1))
        if len(t) != 6 * len(s):
            raise Fatal("uv holds 6 floats per face: (u, v) of each of its three vertices")
        self._check(lib().rt3_bind_mesh_textures(self._ctx, _p(s), _p(t), len(s)))

    # -- the environment map (rt3_set_environment*) -----------------------------------------------------
    def set_environment(self, cube):
        """Sets the cube map every Mode-X ray that leaves the scene reads (rt3_set_environment): a numpy array (6, N, N, 3 | 4), faces +X, -X,
        +Y, -Y, +Z, -Z, row 0 first — the context copies it — or a contiguous (6, N, N, 4) float32 torch tensor on the GPU, copied on
        torch.cuda.current_stream() (rt3_set_environment_device; its texels are not validated)."""
        if type(cube).__module__.startswith("torch"):
            import torch
            if (not cube.is_cuda or cube.dtype != torch.float32 or cube.dim() != 4 or cube.shape[0] != 6 or cube.shape[1] != cube.shape[2] or
                    cube.shape[3] != 4 or not cube.is_contiguous()):
                raise Fatal("a device environment must be a contiguous (6, N, N, 4) float32 tensor on the GPU")
            stream = torch.cuda.current_stream(cube.device).cuda_stream
            self._check(lib().rt3_set_environment_device(self._ctx, C.c_void_p(cube.data_ptr()), int(cube.shape[1]), C.c_void_p(stream or 0)))
            return
        rgba = _cube_rgba(cube)
        self._check(lib().rt3_set_environment(self._ctx, _p(rgba), rgba.shape[1]))

    def clear_environment(self):
        """Removes the map: a miss is the sky again (rt3_clear_environment)."""
        self._check(lib().rt3_clear_environment(self._ctx))

    def environment_size(self):
        """N of the map that is set, 0 when none is (rt3_environment_size)."""
        return int(lib().rt3_environment_size(self._ctx))

    def environment_table(self):
        """The sampling table the device built for the map that is set (rt3_debug_environment_table; built now if no call with FLAG_ENV_SAMPLING
        has built it): (q uint32 (6, M, M), cdf uint64 (6, M, M)), M = min(N, 256) cells per face edge, cdf the inclusive prefix sums of q."""
        n = self.environment_size()
        m = min(n, 256)
        q = np.zeros(max(6 * m * m, 1), np.uint32)
        cdf = np.zeros(max(6 * m * m, 1), np.uint64)
        got = C.c_uint32(0)
        self._check(lib().rt3_debug_environment_table(self._ctx, _p(q), _p(cdf), 6 * m * m, C.byref(got)))
        assert got.value == m
        return q[:6 * m * m].reshape(6, m, m), cdf[:6 * m * m].reshape(6, m, m)

    def light_table(self):
        """The emitters' sampling table the device built for the scene that is set (rt3_debug_light_table; built now if no call with
        FLAG_LIGHT_SAMPLING has built it): (q uint32 (n,), cdf uint64 (n,)), one entry per primitive, faces first and then spheres in the caller's
        order, cdf the inclusive prefix sums of q."""
        got = C.c_uint32(0)
        one_q, one_c = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        rc = lib().rt3_debug_light_table(self._ctx, _p(one_q), _p(one_c), 0, C.byref(got))       # (the count: refused for its capacity, the count set)
        if got.value == 0:
            self._check(rc)
        n = got.value
        q = np.zeros(n, np.uint32)
        cdf = np.zeros(n, np.uint64)
        self._check(lib().rt3_debug_light_table(self._ctx, _p(q), _p(cdf), n, C.byref(got)))
        assert got.value == n
        return q, cdf

    @staticmethod
    def environment_lookup(cube, d):
        """The lookup law on the host (rt3_debug_environment_lookup; no device): cube (6, N, N, 3 | 4), d (3,) or (K, 3) -> float32 (3,) or (K, 3)."""
        return environment_lookup(cube, d)

    # -- camera rays, first-hit AOVs, the linear frame -----------------------------------------------
    def camera_rays(self, camera_c, params, sample_begin=0, sample_count=None):
        """Mode X's primary rays for samples [begin, begin + count) (default: all spp) as a RAY array, sample-major: record
        (s - begin) * npix + pix over the owned pixels (compact tile rows).  Feed them to intersect() to shade or pick."""
        if sample_count is None:
            sample_count = params.spp - sample_begin
        n = lib().rt3_rows_owned(C.byref(params)) * params.width * max(int(sample_count), 0)
        out = np.zeros(n, RAY)
        self._check(lib().rt3_camera_rays(self._ctx, C.byref(camera_c), C.byref(params), sample_begin, sample_count, _p(out)))
        return out

    def camera_rays_device(self, camera_c, params, sample_begin, sample_count, d_out_ptr, stream_ptr=None):
        self._check(lib().rt3_camera_rays_device(self._ctx, C.byref(camera_c), C.byref(params), sample_begin, sample_count,
                                                 C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    def render_aov(self, camera_c, params):
        """First-hit AOVs (rt3_render_aov): an AOV array of shape (rows_owned, width)."""
        rows = lib().rt3_rows_owned(C.byref(params))
        out = np.zeros((rows, params.width), AOV)
        self._check(lib().rt3_render_aov(self._ctx, C.byref(camera_c), C.byref(params), _p(out)))
        return out

    def render_aov_device(self, camera_c, params, d_out_ptr, stream_ptr=None):
        """Asynchronous AOVs into a device buffer of rows_owned * width * 48 bytes (e.g. a torch tensor's data_ptr())."""
        self._check(lib().rt3_render_aov_device(self._ctx, C.byref(camera_c), C.byref(params), C.c_void_p(d_out_ptr),
                                                C.c_void_p(stream_ptr or 0)))

    def render_aov_specular(self, camera_c, params, max_bounces=8, max_fuzz=0.0):
        """Specular-chain AOVs (rt3_render_aov_specular): render_aov with every ray followed through glass and through metals of
        fuzz <= max_fuzz, at most max_bounces times, to the first rough surface — albedo, normal and path length of that end; kind / index of the
        first hit.  max_bounces = 0 is render_aov.  For denoise(), not for the temporal denoisers (they rebuild the first-hit point from depth)."""
        rows = lib().rt3_rows_owned(C.byref(params))
        out = np.zeros((rows, params.width), AOV)
        chain = rt3_aov_chain_params(max_bounces, max_fuzz, 0, 0)
        self._check(lib().rt3_render_aov_specular(self._ctx, C.byref(camera_c), C.byref(params), C.byref(chain), _p(out)))
        return out

    def render_aov_specular_device(self, camera_c, params, d_out_ptr, stream_ptr=None, max_bounces=8, max_fuzz=0.0):
        """rt3_render_aov_specular_device into a device buffer of rows_owned * width * 48 bytes.  The call reads one word back per bounce (it
        stops once every chain has ended), so it is ordered on the stream but waits for it."""
        chain = rt3_aov_chain_params(max_bounces, max_fuzz, 0, 0)
        self._check(lib().rt3_render_aov_specular_device(self._ctx, C.byref(camera_c), C.byref(params), C.byref(chain), C.c_void_p(d_out_ptr),
                                                         C.c_void_p(stream_ptr or 0)))

    def accum_resolve(self, params):
        """The accumulation as a linear float frame (rt3_accum_resolve): float32 (rows_owned, width, 4), (r, g, b, 0)."""
        rows = lib().rt3_rows_owned(C.byref(params))
        out = np.zeros((rows, params.width, 4), np.float32)
        self._check(lib().rt3_accum_resolve(self._ctx, _p(out)))
        return out

    def accum_resolve_device(self, d_out_ptr, stream_ptr=None):
        self._check(lib().rt3_accum_resolve_device(self._ctx, C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    # -- the denoiser -----------------------------------------------------------------------------------
    def denoise(self, colour, aov, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0):
        """The AOV-guided a-trous denoiser (rt3_denoise) of one whole frame, row 0 on top.  numpy: colour float32 (H, W, 4) as accum_resolve
        returns it, aov an (H, W) AOV array -> float32 (H, W, 4), (r, g, b, 0).  torch: a contiguous (H, W, 4) float32 tensor on the GPU and a
        contiguous tensor of the frame's 48-byte rt3_aov records whose first two dimensions are (H, W) (e.g. (H, W, 12) float32) -> a new
        (H, W, 4) float32 tensor, computed on torch.cuda.current_stream()."""
        p = DENOISE_PARAMS(iterations, normal_power, sigma_luminance, sigma_depth)
        if type(colour).__module__.startswith("torch"):
            import torch
            if (not colour.is_cuda or colour.dtype != torch.float32 or colour.dim() != 3 or colour.shape[2] != 4
                    or not colour.is_contiguous()):
                raise Fatal("device colour must be a contiguous (H, W, 4) float32 tensor on the GPU")
            h, w = colour.shape[:2]
            if (not type(aov).__module__.startswith("torch") or not aov.is_cuda or aov.dim() < 2 or tuple(aov.shape[:2]) != (h, w)
                    or aov.numel() * aov.element_size() != h * w * AOV.itemsize or not aov.is_contiguous()):
                raise Fatal("device AOVs must be a contiguous tensor of (H, W) 48-byte records on the GPU")
            out = torch.empty_like(colour)
            stream = torch.cuda.current_stream(colour.device).cuda_stream
            self._check(lib().rt3_denoise_device(self._ctx, w, h, C.c_void_p(colour.data_ptr()), C.c_void_p(aov.data_ptr()), C.byref(p),
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
            return out
        c = np.ascontiguousarray(colour, np.float32)
        a = np.ascontiguousarray(aov)
        if c.ndim != 3 or c.shape[2] != 4 or a.dtype != AOV or a.shape != c.shape[:2]:
            raise Fatal("denoise: colour must be float32 (H, W, 4) and aov an (H, W) AOV array")
        h, w = c.shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        self._check(lib().rt3_denoise(self._ctx, w, h, _p(c), _p(a), C.byref(p), _p(out)))
        return out

    # -- the display transform ---------------------------------------------------------------------------
    def display(self, colour, curve="filmic", transfer="srgb", exposure=1.0, auto=False, key=0.18, white=4.0, trim_low=102, trim_high=51):
        """A linear float frame to RGBA8 words (rt3_display): exposure — given, or with auto=True times key over the frame's trimmed log-average
        luminance —, the tone curve ("clamp" | "reinhard" | "filmic") and the transfer function ("linear" | "gamma2" | "srgb").  numpy: float32
        (H, W, 4) as accum_resolve or denoise return it -> uint32 (H, W), 0xFF | B << 8 | G << 16 | R << 24 as render_path packs.  torch: a contiguous
        (H, W, 4) float32 tensor on the GPU -> a new (H, W) uint32 tensor (int32 bit patterns where torch has no uint32), computed on torch.cuda.current_stream() with no
        host wait.  display(accum_resolve(p), "clamp", "linear" | "gamma2") is render_path's frame."""
        p = display_params(curve, transfer, exposure, auto, key, white, trim_low, trim_high)
        if type(colour).__module__.startswith("torch"):
            import torch
            if (not colour.is_cuda or colour.dtype != torch.float32 or colour.dim() != 3 or colour.shape[2] != 4
                    or not colour.is_contiguous()):
                raise Fatal("device colour must be a contiguous (H, W, 4) float32 tensor on the GPU")
            h, w = colour.shape[:2]
            out = torch.empty((h, w), dtype=getattr(torch, "uint32", torch.int32), device=colour.device)
            stream = torch.cuda.current_stream(colour.device).cuda_stream
            self._check(lib().rt3_display_device(self._ctx, w, h, C.c_void_p(colour.data_ptr()), C.byref(p), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(stream)))
            return out
        c = np.ascontiguousarray(colour, np.float32)
        if c.ndim != 3 or c.shape[2] != 4:
            raise Fatal("display: colour must be float32 (H, W, 4)")
        h, w = c.shape[:2]
        out = np.zeros((h, w), np.uint32)
        self._check(lib().rt3_display(self._ctx, w, h, _p(c), C.byref(p), _p(out)))
        return out

    def display_device(self, width, height, d_rgba_ptr, display_params_c, d_out_ptr, stream_ptr=None):
        """Asynchronous display transform between device buffers (rt3_display_device): width * height float4 in, as many 4-byte words out."""
        self._check(lib().rt3_display_device(self._ctx, width, height, C.c_void_p(d_rgba_ptr), C.byref(display_params_c), C.c_void_p(d_out_ptr),
                                             C.c_void_p(stream_ptr or 0)))

    def display_state(self):
        """What the last display call with auto-exposure left on the device (rt3_debug_display_state; synchronous): (hist uint32 (512,), dark, gain
        float32)."""
        hist = np.zeros(512, np.uint32)
        dark, gain = C.c_uint32(0), C.c_float(0.0)
        self._check(lib().rt3_debug_display_state(self._ctx, _p(hist), C.byref(dark), C.byref(gain)))
        return hist, int(dark.value), np.float32(gain.value)

    # -- display sequences -------------------------------------------------------------------------------
    def display_sequence(self, colour, prev=None, *, curve="filmic", transfer="srgb", exposure=1.0, auto=False, key=0.18, white=4.0, trim_low=102,
                         trim_high=51, adapt=(256, 64), bloom=None):
        """One frame of a sequence through the display transform (rt3_display_sequence) -> (words, exposure).  As display(), with two additions: with
        auto=True the gain follows the sequence — prev is None for the first frame, else the exposure the previous call returned, and the level
        moves adapt = (brighter, darker) / 1024 of the way to this frame's target —, and bloom = (levels, threshold, intensity) adds a bloom pyramid
        before the tone curve (None: no bloom).  numpy: float32 (H, W, 4) -> (uint32 (H, W), an EXPOSURE record); prev an EXPOSURE record.  torch: a
        contiguous (H, W, 4) float32 tensor on the GPU -> (an (H, W) uint32 tensor, a 16-byte int32 (4,) tensor holding the rt3_exposure record), both
        on the GPU, computed on torch.cuda.current_stream() with no host wait; prev such a 16-byte tensor, kept on the device."""
        p = display_sequence_params(curve, transfer, exposure, auto, key, white, trim_low, trim_high, adapt, bloom)
        if type(colour).__module__.startswith("torch"):
            import torch
            if (not colour.is_cuda or colour.dtype != torch.float32 or colour.dim() != 3 or colour.shape[2] != 4
                    or not colour.is_contiguous()):
                raise Fatal("device colour must be a contiguous (H, W, 4) float32 tensor on the GPU")
            if prev is not None and (not type(prev).__module__.startswith("torch") or not prev.is_cuda or not prev.is_contiguous()
                                     or prev.numel() * prev.element_size() != 16):
                raise Fatal("display_sequence: with a device frame prev must be a contiguous 16-byte tensor on the GPU")
            h, w = colour.shape[:2]
            out = torch.empty((h, w), dtype=getattr(torch, "uint32", torch.int32), device=colour.device)
            state = torch.empty(4, dtype=torch.int32, device=colour.device)
            stream = torch.cuda.current_stream(colour.device).cuda_stream
            self._check(lib().rt3_display_sequence_device(self._ctx, w, h, C.c_void_p(colour.data_ptr()), C.byref(p),
                                                          C.c_void_p(prev.data_ptr()) if prev is not None else None, C.c_void_p(state.data_ptr()),
                                                          C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
            return out, state
        c = np.ascontiguousarray(colour, np.float32)
        if c.ndim != 3 or c.shape[2] != 4:
            raise Fatal("display_sequence: colour must be float32 (H, W, 4)")
        h, w = c.shape[:2]
        before = np.array(prev, EXPOSURE).reshape(1) if prev is not None else None
        out, state = np.zeros((h, w), np.uint32), np.zeros(1, EXPOSURE)
        self._check(lib().rt3_display_sequence(self._ctx, w, h, _p(c), C.byref(p), _p(before), _p(state), _p(out)))
        return out, state[0]

    def display_sequence_device(self, width, height, d_rgba_ptr, params_c, d_prev_ptr, d_out_exposure_ptr, d_out_ptr, stream_ptr=None):
        """Asynchronous rt3_display_sequence_device between device buffers: width * height float4 in, as many 4-byte words out, the 16-byte
        rt3_exposure records before (0: none) and after (0: not wanted); the two may be the same buffer.  params_c: a DISPLAY_SEQUENCE_PARAMS."""
        self._check(lib().rt3_display_sequence_device(self._ctx, width, height, C.c_void_p(d_rgba_ptr), C.byref(params_c), C.c_void_p(d_prev_ptr or 0),
                                                      C.c_void_p(d_out_exposure_ptr or 0), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    def display_bloom_state(self):
        """What the last display_sequence call with bloom left on the device (rt3_debug_display_bloom; synchronous): (U_1 float32 (H_1, W_1, 4), B
        float32 (H, W, 4)) — the pyramid's finest plane after the up-sampling sums, and the bloom the composite added, at the frame's size."""
        w, h = C.c_uint32(0), C.c_uint32(0)
        rc = lib().rt3_debug_display_bloom(self._ctx, None, None, 0, C.byref(w), C.byref(h))
        if w.value == 0:
            self._check(rc)
        u1 = np.zeros(((h.value + 1) // 2, (w.value + 1) // 2, 4), np.float32)
        b = np.zeros((h.value, w.value, 4), np.float32)
        self._check(lib().rt3_debug_display_bloom(self._ctx, _p(u1), _p(b), w.value * h.value, C.byref(w), C.byref(h)))
        return u1, b

    def denoise_temporal(self, colour, aov, camera_c, prev=None, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0,
                         alpha=0.2, moments_alpha=0.2, depth_tolerance=2.0, normal_tolerance=0.9, motion=None):
        """One frame of a sequence through the temporal denoiser (rt3_denoise_temporal) -> (out, history).  colour and aov
        as for denoise, camera_c the rt3_camera they were rendered with; prev None for the first frame, else the history of the previous
        call; history = (records, camera): an (H, W) HISTORY array (numpy) or a contiguous (H, W, 12) float32 GPU tensor (torch), and a copy
        of camera_c.  motion: None, or the plane motion() returned for this frame ((H, W, 4) float32, numpy or torch as colour is): pixels of
        primitives that moved are reprojected from where they were (rt3_denoise_temporal_motion).  torch inputs run on
        torch.cuda.current_stream()."""
        p = TEMPORAL_PARAMS(DENOISE_PARAMS(iterations, normal_power, sigma_luminance, sigma_depth), alpha, moments_alpha, depth_tolerance,
                            normal_tolerance)
        return self._denoise_temporal(colour, aov, rt3_camera.from_buffer_copy(bytes(camera_c)), prev, motion, p,
                                      lib().rt3_denoise_temporal_motion, lib().rt3_denoise_temporal_motion_device)

    def denoise_temporal_lens(self, colour, aov, lens, prev=None, motion=None, iterations=5, normal_power=128, sigma_luminance=4.0,
                              sigma_depth=1.0, alpha=0.2, moments_alpha=0.2, depth_tolerance=2.0, normal_tolerance=0.9):
        """denoise_temporal for a frame rendered through a lens (rt3_denoise_temporal_optic) -> (out, (history, lens)): colour
        and aov the whole frame of render_lens / render_lens_aov for `lens`, prev None or what the previous call returned second, motion None
        or the plane motion_lens() returned for this frame.  numpy or torch as denoise_temporal; torch runs on torch.cuda.current_stream()."""
        p = TEMPORAL_PARAMS(DENOISE_PARAMS(iterations, normal_power, sigma_luminance, sigma_depth), alpha, moments_alpha, depth_tolerance,
                            normal_tolerance)
        return self._denoise_temporal(colour, aov, rt3_lens.from_buffer_copy(bytes(lens)), prev, motion, p,
                                      lib().rt3_denoise_temporal_optic, lib().rt3_denoise_temporal_optic_device)

    def _denoise_temporal(self, colour, aov, cam, prev, motion, p, host_fn, device_fn):
        """Both temporal calls: cam is a copy of the frame's view (an rt3_camera or an rt3_lens), host_fn / device_fn the entry points for it."""
        prev_rec, prev_cam = prev if prev is not None else (None, None)
        pc = C.byref(prev_cam) if prev_cam is not None else None
        if type(colour).__module__.startswith("torch"):
            import torch
            if (not colour.is_cuda or colour.dtype != torch.float32 or colour.dim() != 3 or colour.shape[2] != 4
                    or not colour.is_contiguous()):
                raise Fatal("device colour must be a contiguous (H, W, 4) float32 tensor on the GPU")
            h, w = colour.shape[:2]
            for t, what in ((aov, "AOVs"), (prev_rec, "history")):
                if t is None:
                    continue
                if (not type(t).__module__.startswith("torch") or not t.is_cuda or t.dim() < 2 or tuple(t.shape[:2]) != (h, w)
                        or t.numel() * t.element_size() != h * w * 48 or not t.is_contiguous()):
                    raise Fatal("device %s must be a contiguous tensor of (H, W) 48-byte records on the GPU" % what)
            if motion is not None and (not type(motion).__module__.startswith("torch") or not motion.is_cuda or motion.dtype != torch.float32
                                       or tuple(motion.shape) != (h, w, 4) or not motion.is_contiguous()):
                raise Fatal("device motion must be a contiguous (H, W, 4) float32 tensor on the GPU")
            out = torch.empty_like(colour)
            hist = torch.empty((h, w, 12), dtype=torch.float32, device=colour.device)
            stream = torch.cuda.current_stream(colour.device).cuda_stream
            self._check(device_fn(
                self._ctx, w, h, C.byref(cam), C.c_void_p(colour.data_ptr()), C.c_void_p(aov.data_ptr()), pc,
                C.c_void_p(prev_rec.data_ptr()) if prev_rec is not None else None,
                C.c_void_p(motion.data_ptr()) if motion is not None else None, C.byref(p), C.c_void_p(out.data_ptr()),
                C.c_void_p(hist.data_ptr()), C.c_void_p(stream)))
            return out, (hist, cam)
        c = np.ascontiguousarray(colour, np.float32)
        a = np.ascontiguousarray(aov)
        if c.ndim != 3 or c.shape[2] != 4 or a.dtype != AOV or a.shape != c.shape[:2]:
            raise Fatal("denoise_temporal: colour must be float32 (H, W, 4) and aov an (H, W) AOV array")
        h, w = c.shape[:2]
        pr = None
        if prev_rec is not None:
            pr = np.ascontiguousarray(prev_rec)
            if pr.dtype != HISTORY or pr.shape != (h, w):
                raise Fatal("denoise_temporal: the previous history must be an (H, W) HISTORY array")
        mo = None
        if motion is not None:
            mo = np.ascontiguousarray(motion, np.float32)
            if mo.shape != (h, w, 4):
                raise Fatal("denoise_temporal: motion must be float32 (H, W, 4)")
        out = np.zeros((h, w, 4), np.float32)
        hist = np.zeros((h, w), HISTORY)
        self._check(host_fn(self._ctx, w, h, C.byref(cam), _p(c), _p(a), pc, _p(pr), _p(mo), C.byref(p), _p(out), _p(hist)))
        return out, (hist, cam)

    def motion(self, aov, camera_c, prev_center_radius=None, prev_vertices=None):
        """The motion plane of one frame (rt3_motion) -> (H, W, 4) float32, (mx, my, mz, moved) per pixel.  The scene on this
        renderer is the frame's own, aov its AOVs and camera_c its camera; prev_center_radius ((n_spheres, 4)) and prev_vertices
        ((n_vertices, 4), the merged vertices as mesh_download returns them) are the previous frame's, None for a class that did not move.
        numpy: aov an (H, W) AOV array.  torch: a contiguous tensor of (H, W) 48-byte records and contiguous float32 GPU tensors for the
        previous arrays -> a new tensor, computed on torch.cuda.current_stream()."""
        return self._motion(aov, rt3_camera.from_buffer_copy(bytes(camera_c)), prev_center_radius, prev_vertices, lib().rt3_motion,
                            lib().rt3_motion_device)

    def motion_lens(self, aov, lens, prev_center_radius=None, prev_vertices=None):
        """motion for a frame rendered through a lens (rt3_motion_optic): aov the AOVs of render_lens_aov for `lens`; the
        shown point lies on the lens's centre ray.  numpy or torch as motion."""
        return self._motion(aov, rt3_lens.from_buffer_copy(bytes(lens)), prev_center_radius, prev_vertices, lib().rt3_motion_optic,
                            lib().rt3_motion_optic_device)

    def _motion(self, aov, cam, prev_center_radius, prev_vertices, host_fn, device_fn):
        """Both motion calls: cam is a copy of the frame's view (an rt3_camera or an rt3_lens), host_fn / device_fn the entry points for it."""
        if type(aov).__module__.startswith("torch"):
            import torch
            if not aov.is_cuda or aov.dim() < 2 or aov.numel() * aov.element_size() != aov.shape[0] * aov.shape[1] * 48 or not aov.is_contiguous():
                raise Fatal("device AOVs must be a contiguous tensor of (H, W) 48-byte records on the GPU")
            h, w = aov.shape[:2]
            ptrs = []
            for t, what in ((prev_center_radius, "prev_center_radius"), (prev_vertices, "prev_vertices")):
                if t is None:
                    ptrs += [None, 0]
                    continue
                if (not type(t).__module__.startswith("torch") or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 4
                        or not t.is_contiguous()):
                    raise Fatal("device %s must be a contiguous (N, 4) float32 tensor on the GPU" % what)
                ptrs += [C.c_void_p(t.data_ptr()), t.shape[0]]
            out = torch.empty((h, w, 4), dtype=torch.float32, device=aov.device)
            stream = torch.cuda.current_stream(aov.device).cuda_stream
            self._check(device_fn(self._ctx, w, h, C.byref(cam), C.c_void_p(aov.data_ptr()), *ptrs, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
            return out
        a = np.ascontiguousarray(aov)
        if a.dtype != AOV or a.ndim != 2:
            raise Fatal("motion: aov must be an (H, W) AOV array")
        h, w = a.shape
        ps = None if prev_center_radius is None else np.ascontiguousarray(prev_center_radius, np.float32).reshape(-1, 4)
        pv = None if prev_vertices is None else np.ascontiguousarray(prev_vertices, np.float32).reshape(-1, 4)
        out = np.zeros((h, w, 4), np.float32)
        self._check(host_fn(self._ctx, w, h, C.byref(cam), _p(a), _p(ps), 0 if ps is None else len(ps), _p(pv), 0 if pv is None else len(pv), _p(out)))
        return out

    def set_sample_storage_cap(self, nbytes):
        self._check(lib().rt3_set_sample_storage_cap(self._ctx, nbytes))

    def stats(self):
        s = rt3_stats()
        self._check(lib().rt3_get_stats(self._ctx, C.byref(s)))
        return s

    def force_plain_mode_r(self, on):
        self._check(lib().rt3_debug_force_plain_mode_r(self._ctx, 1 if on else 0))

    def debug_arith(self, a, b):
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        n = len(a)
        outs = [np.zeros(n, np.float32) for _ in range(5)] + [np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)]
        self._check(lib().rt3_debug_arith(self._ctx, _p(a), _p(b), n, *[_p(o) for o in outs]))
        return outs


    def debug_primary_lists(self, cam, params):
        """The strip lists of the current sphere scene for (cam, params): a (groups of 64 owned pixels, row blocks) uint32 array, bit b of
        word k = sphere 32 k + b (tests only)."""
        ng, nb = C.c_uint32(0), C.c_uint32(0)
        npix = rows_owned(params) * params.width
        out = np.zeros((-(-npix // 64), 16), np.uint32)
        self._check(lib().rt3_debug_primary_lists(self._ctx, C.byref(cam), C.byref(params), _p(out), out.size, C.byref(ng), C.byref(nb)))
        return out.reshape(-1)[:ng.value * nb.value].reshape(ng.value, nb.value).copy()


def sphere_plan(center_radius):
    """Tests: what the host upload decides for these (n, 4) records (rt3_debug_sphere_plan; no device): the filter centre (3 float32) and the
    direct list (sorted uint32)."""
    cr = np.ascontiguousarray(center_radius, np.float32).reshape(-1, 4)
    centre = np.zeros(3, np.float32)
    direct = np.zeros(4, np.uint32)
    n = lib().rt3_debug_sphere_plan(_p(cr), len(cr), _p(centre), _p(direct))
    return centre, np.sort(direct[:n])


def initialize_renderer(device=0):
    """RayTracer::initialize_renderer (Renderer.hpp:63): the link-time factory; here it always builds the HIP backend."""
    return HipRenderer(device)


def debug_ctr_table():
    """The counter-hash table of k_trace_mfma32's render form as the library computes it on the host: (rows, 4) uint32 (tests only; no device)."""
    rows = lib().rt3_debug_ctr_table(None, 0)
    out = np.zeros((rows, 4), np.uint32)
    lib().rt3_debug_ctr_table(_p(out), rows)
    return out


def rows_owned(params):
    return lib().rt3_rows_owned(C.byref(params))


def row_of_local(params, local_row):
    return lib().rt3_row_of_local(C.byref(params), local_row)


def deinterleave(tiles, params_list, height, width):
    """Assembles the full frame from the compact per-shard row buffers (the host side of the RCCL gather)."""
    frame = np.zeros((height, width), np.uint32)
    for tile, p in zip(tiles, params_list):
        for r in range(tile.shape[0]):
            frame[row_of_local(p, r)] = tile[r]
    return frame
