"""ctypes binding of libnexoclom_hip.so (include/nexoclom_hip.h) -- the only door to the GPU.

There is no CPU fallback: if the library is missing or no gfx950 device is visible, every
entry point raises.  Arrays cross the boundary as C-contiguous float64 NumPy buffers.
"""
import ctypes as C
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NEXOCLOM_HIP_LIB: load another build of the same library (installation elsewhere, experiments)
LIB_PATH = os.environ.get('NEXOCLOM_HIP_LIB') or os.path.join(_HERE, 'lib', 'libnexoclom_hip.so')
_dp, _fp, _cp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_char)
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_u8p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
NXC_MAX_LINES = 4
NXC_RUN_IMAGE = 1
NXC_UNIQUE_ID_BYTES = 128

ABI_VERSION = 3


NXC_ERR_HIP, NXC_ERR_ARG, NXC_ERR_NO_DEVICE, NXC_ERR_RCCL, NXC_ERR_STATE, NXC_ERR_NOMEM, \
    NXC_ERR_INCOMPLETE = -1, -2, -3, -4, -5, -6, -7
NXC_ERR_OVERFLOW = -8
FIT_WEIGHT_MODES = {None: 0, 'dist': 1, 'dist2': 2, 'sigma': 3}


class HipError(RuntimeError):
    """An nxc_* call failed; ``code`` is its NXC_ERR_* status (None when raised by the binding)."""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class nxc_forces(C.Structure):
    _fields_ = [('GM', C.c_double), ('vrplanet', C.c_double), ('photo', C.c_double),
                ('lifetime', C.c_double), ('gravity', C.c_int32), ('radpres', C.c_int32),
                ('has_photo', C.c_int32), ('reserved', C.c_int32), ('n_tab', C.c_int64),
                ('v_tab', _dp), ('a_tab', _dp)]


class nxc_image_desc(C.Structure):
    _fields_ = [('M', C.c_double*9), ('vrplanet', C.c_double), ('apix_cm2', C.c_double),
                ('quantity', C.c_int32), ('n_lines', C.c_int32), ('downcast_f32', C.c_int32),
                ('reserved', C.c_int32), ('nx', C.c_int64), ('nz', C.c_int64),
                ('xedges', _dp), ('zedges', _dp), ('line_n', C.c_int64*NXC_MAX_LINES),
                ('line_v', _dp*NXC_MAX_LINES), ('line_g', _dp*NXC_MAX_LINES)]


class nxc_los_desc(C.Structure):
    _fields_ = [('dphi', C.c_double), ('sin_dphi', C.c_double), ('sin_2dphi', C.c_double),
                ('cos_threshold', C.c_double), ('vrplanet', C.c_double), ('unit_cm', C.c_double),
                ('n_lines', C.c_int32), ('reserved', C.c_int32),
                ('line_n', C.c_int64*NXC_MAX_LINES), ('line_v', _dp*NXC_MAX_LINES),
                ('line_g', _dp*NXC_MAX_LINES), ('n_ladder', C.c_int64), ('ladder', _dp)]


class nxc_density_desc(C.Structure):
    _fields_ = [('origin', C.c_double*3), ('h', C.c_double), ('dr', C.c_double),
                ('dims', C.c_int64*3), ('n_points', C.c_int64), ('points', _dp),
                ('cell_start', _i32p)]


class nxc_density_spectrum_desc(C.Structure):
    _fields_ = [('nv', C.c_int64), ('s_lo', C.c_double), ('s_hi', C.c_double),
                ('cos_half', C.c_double), ('all_sky', C.c_int32), ('reserved', C.c_int32),
                ('n_frames', C.c_int64), ('frames', _dp)]


class nxc_camera_desc(C.Structure):
    _fields_ = [('o', C.c_double*3), ('C', C.c_double*9), ('vrplanet', C.c_double),
                ('pix_area_cm2', C.c_double), ('quantity', C.c_int32), ('n_lines', C.c_int32),
                ('nx', C.c_int64), ('nz', C.c_int64), ('uedges', _dp), ('vedges', _dp),
                ('line_n', C.c_int64*NXC_MAX_LINES), ('line_v', _dp*NXC_MAX_LINES),
                ('line_g', _dp*NXC_MAX_LINES)]


class nxc_shell_desc(C.Structure):
    _fields_ = [('vrplanet', C.c_double), ('r_lo', C.c_double), ('r_hi', C.c_double),
                ('quantity', C.c_int32), ('n_lines', C.c_int32), ('nlon', C.c_int64),
                ('nlat', C.c_int64), ('nalt', C.c_int64), ('lon_edges', _dp), ('mu_edges', _dp),
                ('line_n', C.c_int64*NXC_MAX_LINES), ('line_v', _dp*NXC_MAX_LINES),
                ('line_g', _dp*NXC_MAX_LINES)]


class nxc_source_map_desc(C.Structure):
    _fields_ = [('nlon', C.c_int64), ('nlat', C.c_int64), ('nvel', C.c_int64),
                ('nalt', C.c_int64), ('naz', C.c_int64), ('tile', C.c_int64), ('r_km', C.c_double),
                ('alt_edges', _dp), ('az_edges', _dp), ('lon_edges', _dp), ('lat_edges', _dp),
                ('point_lon', _dp), ('point_lat', _dp), ('point_cos', _dp), ('threshold', _dp),
                ('n_seg', C.c_int64), ('seg', _i32p),
                ('seg_off', _i32p)]


class nxc_fit_desc(C.Structure):
    _fields_ = [('n_spectra', C.c_int64), ('weight_mode', C.c_int32), ('reserved', C.c_int32),
                ('position', _dp), ('ratio', _dp), ('weight', _dp),
                ('mask', _u8p)]


class nxc_source_desc(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ('endtime', 'exobase', 'sinlat0', 'sinlat1', 'lon0', 'lon1', 'vprob', 'vwidth',
                 'unit_km', 'sinalt0', 'sinalt1', 'az0', 'az1')] + \
               [(k, C.c_int32) for k in ('random_time', 'speed_type', 'angular_type', 'is_planet')] + \
               [('seed', C.c_uint64), ('first_index', C.c_int64), ('spatial_type', C.c_int32),
                ('reserved', C.c_int32), ('n_speed', C.c_int64), ('speed_cdf', _dp),
                ('speed_v', _dp), ('map_nlon', C.c_int64), ('map_nlat', C.c_int64), ('map', _dp),
                ('generator', C.c_int32), ('reserved2', C.c_int32), ('pcg_state', C.c_uint64*2),
                ('pcg_inc', C.c_uint64*2), ('pcg_n', C.c_int64), ('pcg_row0', C.c_int64),
                ('dest_offset', C.c_int64), ('dest_total', C.c_int64), ('map_cdf', _dp)] + \
               [(k, C.c_double) for k in ('map_lon0', 'map_lon1', 'map_s0', 'map_s1', 't0', 't1')] + \
               [('nx', C.c_int64), ('ny', C.c_int64), ('tx', _dp), ('ty', _dp), ('coef', _dp),
                ('n_node_speed', C.c_int64), ('node_speed_cdf', _dp), ('node_speed_v', _dp),
                ('n_node_alt', C.c_int64), ('node_alt_cdf', _dp), ('node_alt', _dp),
                ('n_node_az', C.c_int64), ('node_az_cdf', _dp), ('node_az', _dp)]


class nxc_bounce_desc(C.Structure):
    _fields_ = [('GM', C.c_double), ('unit_km', C.c_double), ('accomfactor', C.c_double),
                ('stickcoef', C.c_double), ('A', C.c_double*3), ('t0', C.c_double),
                ('t1', C.c_double), ('temp_dependent', C.c_int32), ('reserved', C.c_int32),
                ('nx', C.c_int64), ('ny', C.c_int64), ('tx', _dp), ('ty', _dp), ('coef', _dp),
                ('seed', C.c_uint64)]


class nxc_stick_map_desc(C.Structure):
    _fields_ = [('nlon', C.c_int64), ('nlat', C.c_int64), ('lon', _dp), ('lat', _dp), ('coef', _dp)]


class nxc_bodies_desc(C.Structure):
    _fields_ = [('n_moons', C.c_int32), ('chx_on', C.c_int32), ('gm', C.c_double*4),
                ('radius', C.c_double*4), ('a', C.c_double*4), ('omega', C.c_double*4),
                ('phi', C.c_double*4), ('t0', C.c_double), ('chx_k0', C.c_double),
                ('chx_rho0', C.c_double), ('chx_width', C.c_double), ('chx_height', C.c_double),
                ('chx_omega', C.c_double)]


class nxc_frame_desc(C.Structure):
    _fields_ = [('omega', C.c_double), ('M', C.c_double*3), ('U', C.c_double*3),
                ('scale', C.c_double)]


class nxc_counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ('particle_steps', 'samples', 'samples_binned', 'nonfinite', 'bad_step',
                 'neg_frac', 'unfinished', 'wave_trips')]


# The argument types of every function include/nexoclom_hip.h declares, in the header's order of
# sections.  load_library() hands them to ctypes, which then converts and checks each call;
# tests/test_abi.py holds them against the prototypes of the header itself.
_int, _i32, _i64, _u32, _dbl = C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_double
_h = C.c_void_p                          # nxc_handle *, nxc_rows *, nxc_pairs *, void *
_out = C.POINTER(C.c_void_p)             # nxc_rows **, nxc_pairs **, nxc_handle **
_los_results = (_i64, _dp, _i64p, _u8p, _i64, _i64p, _i64p)   # n_index .. n_used


def _sample_entries(name, ncols, head=(), index=False, tail=()):
    """The three entries that read stored samples: ``name`` (P rows of ``ncols`` double columns),
    ``name``_f32 (float columns) and ``name``_rows (a row store, first, count).  ``head`` and
    ``tail`` are the arguments around the samples; ``index``: the samples come with their packet
    index (host columns: an int64 column; rows: the shift of the store's own)."""
    host = {name + suffix: (_h, *head, _i64, *[col]*ncols, *[_i64p]*index, *tail)
            for suffix, col in (('', _dp), ('_f32', _fp))}
    return {**host, name + '_rows': (_h, *head, _h, _i64, _i64, *[_i64]*index, *tail)}


def _desc(struct):
    return (_h, C.POINTER(struct))


SIGNATURES = {
    'nxc_abi_version': (),
    'nxc_device_count': (C.POINTER(_int),),
    'nxc_last_error_string': (),
    'nxc_create': (_int, _out),
    'nxc_destroy': (_h,),
    'nxc_device_name': (_h, _cp, _int),
    'nxc_device_bus_id': (_h, _cp, _int),
    'nxc_synchronize': (_h,),
    'nxc_mem_info': (_h, _u64p, _u64p),
    'nxc_set_forces': _desc(nxc_forces),
    'nxc_set_image': _desc(nxc_image_desc),
    'nxc_set_bounce': _desc(nxc_bounce_desc),
    'nxc_set_first_index': (_h, _i64),
    'nxc_set_stick_map': _desc(nxc_stick_map_desc),
    'nxc_set_bodies': _desc(nxc_bodies_desc),
    'nxc_state': (_h, _i64, *[_dp]*8),
    'nxc_rk5_step': (_h, _i64, _dp, _dp, _dp, _dp),
    'nxc_packets_upload': (_h, _i64, _dp),
    'nxc_packets_upload_pieces': (_h, _i32, _i64p, C.POINTER(_dp)),
    'nxc_image_clear': (_h,),
    'nxc_image_download': (_h, _dp, _u64p),
    'nxc_counters_get': _desc(nxc_counters),
    'nxc_last_kernel_ms': (_h, _fp),
    'nxc_packets_sample': (*_desc(nxc_source_desc), _i64, _dp),
    'nxc_integrate_const': (_h, _dbl, _i64, _dbl, _u32, _dp, _i64, _dp, _i64p),
    'nxc_integrate_const_rows': (_h, _dbl, _i64, _dbl, _i64p, _i64p),
    'nxc_rows_fetch': (_h, _dp),
    'nxc_rows_fetch_f32': (_h, _fp),
    'nxc_rows_build': (_h, _int, _out),
    'nxc_rows_info': (_h, _i64p, _i32p),
    'nxc_rows_download': (_h, _h, _i64, _i64, _h, _h),
    'nxc_rows_free': (_h, _h),
    'nxc_integrate_const_async': (_h, _dbl, _i64, _dbl, _u32),
    'nxc_integrate_const_streamed': (_h, _i64, _dp, _i32, _dbl, _i64, _dbl, _u32),
    'nxc_integrate_var': (_h, _dbl, _dbl, _i64, _dp, _dp),
    'nxc_integrate_var_resident': (_h, _dbl, _dbl, _i64, _dp),
    'nxc_var_rows_build': (_h, _int, _int, _out, _u8p),
    **_sample_entries('nxc_image_accumulate', 5),
    'nxc_image_mode': (_h, _int, _int, _i64),
    **_sample_entries('nxc_los_accumulate', 5, (C.POINTER(nxc_los_desc), _i64, _dp), True,
                      _los_results),
    'nxc_density_set': _desc(nxc_density_desc),
    **_sample_entries('nxc_density_accumulate', 4),
    'nxc_density_download': (_h, _dp, _dp),
    'nxc_density_moments_enable': (_h, _int),
    **_sample_entries('nxc_density_moments_accumulate', 7),
    'nxc_density_moments_download': (_h, _dp),
    'nxc_density_spectrum_enable': _desc(nxc_density_spectrum_desc),
    **_sample_entries('nxc_density_spectrum_accumulate', 7),
    'nxc_density_spectrum_download': (_h, _dp),
    'nxc_density_ages_enable': (_h, _i64, _dbl, _dbl, _dbl),
    **_sample_entries('nxc_density_ages_accumulate', 5),
    'nxc_density_ages_download': (_h, _dp),
    'nxc_density_ages_upload': (_h, _dp),
    'nxc_density_ages_apply': (_h, _i64, _dp, _dp),
    'nxc_camera_set': _desc(nxc_camera_desc),
    **_sample_entries('nxc_camera_accumulate', 5),
    'nxc_camera_download': (_h, _dp, _u64p),
    'nxc_image_moments_enable': (_h, _int),
    **_sample_entries('nxc_image_moments_accumulate', 7),
    'nxc_image_moments_download': (_h, _dp),
    'nxc_camera_moments_enable': (_h, _int),
    **_sample_entries('nxc_camera_moments_accumulate', 7),
    'nxc_camera_moments_download': (_h, _dp),
    'nxc_image_cube_enable': (_h, _i64, _dbl, _dbl),
    **_sample_entries('nxc_image_cube_accumulate', 7),
    'nxc_image_cube_download': (_h, _dp),
    'nxc_camera_cube_enable': (_h, _i64, _dbl, _dbl),
    **_sample_entries('nxc_camera_cube_accumulate', 7),
    'nxc_camera_cube_download': (_h, _dp),
    'nxc_shell_set': _desc(nxc_shell_desc),
    **_sample_entries('nxc_shell_accumulate', 5),
    'nxc_shell_download': (_h, _dp, _u64p, _dp),
    'nxc_shell_moments_enable': (_h, _int),
    **_sample_entries('nxc_shell_moments_accumulate', 7),
    'nxc_shell_moments_download': (_h, _dp),
    'nxc_shell_ages_enable': (_h, _i64, _dbl, _dbl, _dbl),
    **_sample_entries('nxc_shell_ages_accumulate', 6),
    'nxc_shell_ages_download': (_h, _dp),
    'nxc_shell_ages_upload': (_h, _dp),
    'nxc_shell_ages_apply': (_h, _i64, _dp, _dp),
    'nxc_los_profile_enable': (_h, _i64, _i64, _dbl, _dbl),
    **_sample_entries('nxc_los_profile_accumulate', 7, (C.POINTER(nxc_los_desc), _i64, _dp), True,
                      _los_results),
    'nxc_los_profile_download': (_h, _dp, _dp),
    'nxc_source_map_set': _desc(nxc_source_map_desc),
    'nxc_source_map_accumulate': (_h, _i64, *[_dp]*6, _i32p, _dp, _i32, _dbl, _dp),
    'nxc_source_map_download': (_h, _dp, _dp),
    'nxc_pairs_create': (_h, _i64, _out),
    'nxc_pairs_free': (_h, _h),
    'nxc_pairs_count': (_h, _i64p),
    'nxc_pairs_download': (_h, _h, _i64p, _i64p),
    'nxc_los_set_pairs': (_h, _h),
    'nxc_fit_set': _desc(nxc_fit_desc),
    **_sample_entries('nxc_fit_source', 5, index=True),
    'nxc_fit_packets': (_h, _h, _i64, _dp, _dp, _i32p, _dp, _dp),
    'nxc_fit_radiance': (_h, _h, C.POINTER(nxc_los_desc)),
    'nxc_fit_rows': (_h, _int, _out, _i64p),
    'nxc_fit_download': (_h, _dp),
    'nxc_comm_unique_id': (_u8p,),
    'nxc_comm_init': (_h, _u8p, _int, _int),
    'nxc_comm_destroy': (_h,),
    'nxc_image_allreduce': (_h,),
    'nxc_allreduce_max_f64': (_h, _dp),
    'nxc_allreduce_sum_f64': (_h, _dp),
    'nxc_barrier': (_h,),
    'nxc_allreduce_f64': (_h, _dp, _i64),
    'nxc_comm_set_timeout': (_h, _dbl),
    'nxc_comm_abort': (_h,),
    'nxc_comm_request_abort': (_h,),
    'nxc_comm_test_stall': (_h, _dbl),
    'nxc_stream_copy_gbs': (_h, _i64, _int, _dp),
    'nxc_shader_clock_mhz': (_h, _dp),
    'nxc_pcg64_uniforms': (_h, _u64p, _u64p, _i64, _i64, _i64, _i32, _dp),
    'nxc_math_batch': (_h, _int, _i64, _dp, _dp, _dp),
    'nxc_frame_rows': (*_desc(nxc_frame_desc), _h, _i64, _i64, _out),
    'nxc_frame_columns': (*_desc(nxc_frame_desc), _i64, *[_dp]*7, _dp),
    'nxc_frame_columns_f32': (*_desc(nxc_frame_desc), _i64, *[_fp]*7, _fp),
    'nxc_image_ages_enable': (_h, _i64, _dbl, _dbl, _dbl),
    **_sample_entries('nxc_image_ages_accumulate', 6),
    'nxc_image_ages_download': (_h, _dp),
    'nxc_image_ages_upload': (_h, _dp),
    'nxc_image_ages_apply': (_h, _i64, _dp, _dp),
    'nxc_camera_ages_enable': (_h, _i64, _dbl, _dbl, _dbl),
    **_sample_entries('nxc_camera_ages_accumulate', 6),
    'nxc_camera_ages_download': (_h, _dp),
    'nxc_camera_ages_upload': (_h, _dp),
    'nxc_camera_ages_apply': (_h, _i64, _dp, _dp),
    'nxc_los_ages_enable': (_h, _i64, _i64, _dbl, _dbl, _dbl),
    **_sample_entries('nxc_los_ages_accumulate', 6, (C.POINTER(nxc_los_desc), _i64, _dp), True,
                      _los_results),
    'nxc_los_ages_download': (_h, _dp),
}
RESTYPES = {'nxc_last_error_string': C.c_char_p}       # every other function returns an int status
EXPORTS = tuple(SIGNATURES)

_lib = None


def ages_apply_plan(planes, ne, lds_bytes=64*1024):
    """(stride, run, chunk) of a workgroup of k_ages_apply for ``planes`` = na + 2 planes and
    ``ne`` epochs on a device with ``lds_bytes`` of LDS per workgroup: records from one pixel to the
    next in LDS, pixels per workgroup, epochs per workgroup -- ages_apply_plan of
    csrc/nxc_ages_check.hpp in Python, for what wants to know how often a call reads the block
    (ceil(ne / chunk) times); tests/test_age_cube_cpu.py holds it against the C++.  None: one pixel
    and one epoch do not fit."""
    stride = planes | 1
    least = stride*16 + planes*8
    if planes < 3 or ne < 1 or least > lds_bytes:
        return None
    budget = min(lds_bytes, max(32*1024, least))
    chunk = max(1, min(ne, 64, ((budget - stride*16)//2)//(planes*8)))
    run = max(1, min(256, (budget - planes*chunk*8)//(stride*16)))
    return stride, run, chunk


def load_library():
    """dlopen the in-tree library (building nothing); raises HipError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(f'{LIB_PATH} not found: build it with `python -m nexoclom_amd.build` '
                       '(there is no CPU fallback for the hot path)')
    # several processes on one node (RCCL, shared device memory): this pool's host driver only
    # supports dmabuf IPC; without the setting ncclCommInitRank fails in hipIpcGetMemHandle.  Read
    # by the runtime when it initialises, i.e. at the first HIP call -- none has been made yet.
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    lib = C.CDLL(LIB_PATH)
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    for name, argtypes in SIGNATURES.items():
        if name not in missing:
            entry = getattr(lib, name)
            entry.argtypes, entry.restype = argtypes, RESTYPES.get(name, C.c_int)
    # (an explicitly named build -- experiments comparing library versions -- may lack the newest
    # entry points; the in-tree library may not)
    if missing and not os.environ.get('NEXOCLOM_HIP_LIB'):
        raise HipError(f'{LIB_PATH} lacks {missing}: rebuild with `python -m nexoclom_amd.build`')
    if lib.nxc_abi_version() != ABI_VERSION:
        raise HipError(f'libnexoclom_hip.so has ABI version {lib.nxc_abi_version()}, this binding '
                       f'is written for {ABI_VERSION}: rebuild with `python -m nexoclom_amd.build`')
    _lib = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def pcg64_words(seed):
    """(state, inc) of numpy.random.default_rng(seed)'s bit generator as {high, low} 64-bit words
    (what nxc_source_desc.pcg_state / pcg_inc take)."""
    st = np.random.PCG64(seed).state['state']
    mask = (1 << 64) - 1
    return ((C.c_uint64*2)(st['state'] >> 64, st['state'] & mask),
            (C.c_uint64*2)(st['inc'] >> 64, st['inc'] & mask))


def _p(a):
    return a.ctypes.data_as(_dp)


def device_count():
    lib = load_library()
    n = C.c_int(0)
    rc = lib.nxc_device_count(C.byref(n))
    if rc != 0:
        return 0
    return n.value


class RowStore:
    """Compact trajectory rows that stay in HBM (an ``nxc_rows``): the nine columns time, x, y, z,
    vx, vy, vz, frac, lossfrac and the packet-index column of ``total`` live records, float32 /
    int32 when ``narrow`` (what the reference's save() stores) or float64 / int64.  Views of it
    (row ranges) feed the image and line-of-sight kernels without touching the host."""

    def __init__(self, ctx, handle):
        self.ctx, self._r = ctx, handle
        self.owners = weakref.WeakSet()       # the Outputs whose rows these are
        self._lock = threading.RLock()        # a file writer may be reading while the store is spilled
        total, f32 = C.c_int64(0), C.c_int32(0)
        ctx._check(ctx.lib.nxc_rows_info(handle, C.byref(total), C.byref(f32)))
        self.total, self.narrow = int(total.value), bool(f32.value)

    @property
    def nbytes(self):
        return self.total * (9*4 + 4 if self.narrow else 9*8 + 8)

    def download(self, first=0, count=None, index=True):
        """(rows (9, count), index (count,) | None) of the row range as host arrays."""
        count = self.total - first if count is None else int(count)
        rows = np.empty((9, count), dtype=np.float32 if self.narrow else np.float64)
        idx = np.empty(count, dtype=np.int32 if self.narrow else np.int64) if index else None
        with self._lock:
            if self._r is None:
                raise HipError('the row store has been freed')
            self.ctx._check(self.ctx.lib.nxc_rows_download(
                self.ctx._h, self._r, first, count,
                rows.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p) if index else None))
        return rows, idx

    def free(self):
        with self._lock:
            if self._r is not None and getattr(self.ctx, '_h', None):
                self.ctx.lib.nxc_rows_free(self.ctx._h, self._r)
            self._r = None

    def spill(self):
        """Leave HBM: every owner first takes its rows to the host."""
        for owner in list(self.owners):
            owner._spill()
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PairList:
    """A device list of (spectrum, row) pairs (an ``nxc_pairs``): what a line-of-sight pass found
    with weight > 0, when it is passed as ``los_accumulate(..., pairs=...)``."""

    def __init__(self, ctx, capacity):
        self.ctx, self.capacity = ctx, int(capacity)
        self._p = C.c_void_p()
        ctx._check(ctx.lib.nxc_pairs_create(ctx._h, self.capacity, C.byref(self._p)))

    @property
    def count(self):
        n = C.c_int64(0)
        self.ctx._check(self.ctx.lib.nxc_pairs_count(self._p, C.byref(n)))
        return int(n.value)

    def download(self):
        """(2, n) int64: spectrum, row of every pair, in the order the pass wrote them."""
        n = self.count
        out = np.zeros((2, n), dtype=np.int64)
        self.ctx._check(self.ctx.lib.nxc_pairs_download(self.ctx._h, self._p,
                                                        out[0].ctypes.data_as(_i64p),
                                                        out[1].ctypes.data_as(_i64p)))
        return out

    def free(self):
        if self._p and getattr(self.ctx, '_h', None):
            self.ctx.lib.nxc_pairs_free(self.ctx._h, self._p)
        self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One device + stream + tables + resident packets/image (an ``nxc_handle``)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self._h = C.c_void_p()
        self._check(self.lib.nxc_create(device, C.byref(self._h)))
        self.device = device
        self.n_packets = 0
        self.image_shape = None
        # 'image' / 'camera' -> the token of the product whose total the resident age block holds;
        # whatever changes the block (a set, a clear, an enable, an ages pass, an upload) drops it
        self.ages_owner = {}
        self._stores = []              # resident RowStores, oldest first (weak references)

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            msg = self.lib.nxc_last_error_string()
            raise HipError(f'nexoclom_hip error {rc}: {msg.decode() if msg else "?"}', rc)

    def make_room(self, need):
        """Before ``need`` bytes of row store (+ scratch) are allocated: spill the oldest resident
        stores to their owners' host memory until they fit (their Outputs keep working from the
        host copy)."""
        alive = [ref for ref in self._stores if ref() is not None and ref()._r is not None]
        self._stores = alive
        while alive and self.mem_info()[0] < need + (1 << 30):
            alive.pop(0)().spill()

    def close(self):
        for ref in getattr(self, '_stores', ()):
            store = ref()
            if store is not None:
                store.free()
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.nxc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._check(self.lib.nxc_device_name(self._h, buf, 256))
        return buf.value.decode()

    def bus_id(self):
        buf = C.create_string_buffer(64)
        self._check(self.lib.nxc_device_bus_id(self._h, buf, 64))
        return buf.value.decode()

    def synchronize(self):
        try:
            self._check(self.lib.nxc_synchronize(self._h))
        except HipError as exc:
            if exc.code == NXC_ERR_INCOMPLETE:
                self.n_packets = 0
            raise

    def mem_info(self):
        """(free, total) bytes of device memory."""
        free, total = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.nxc_mem_info(self._h, C.byref(free), C.byref(total)))
        return int(free.value), int(total.value)

    # -- set-up -----------------------------------------------------------------------------
    def set_forces(self, GM, vrplanet, gravity=True, radpres=True, lifetime=0.0, photo=None,
                   v_tab=None, a_tab=None):
        f = nxc_forces()
        f.GM, f.vrplanet = float(GM), float(vrplanet)
        f.photo = 0.0 if photo is None else float(photo)
        f.lifetime = float(lifetime)
        f.gravity, f.radpres, f.has_photo = int(bool(gravity)), int(bool(radpres)), int(photo is not None)
        if radpres:
            v, a = _f64(v_tab), _f64(a_tab)
            if v.shape != a.shape or v.ndim != 1:
                raise ValueError('v_tab and a_tab must be 1-D arrays of equal length')
            f.n_tab, f.v_tab, f.a_tab = len(v), _p(v), _p(a)
        self._check(self.lib.nxc_set_forces(self._h, C.byref(f)))

    def set_image(self, M, vrplanet, apix_cm2, quantity, xedges, zedges, g_tables=(),
                  downcast_f32=False):
        d = nxc_image_desc()
        d.M = (C.c_double*9)(*np.asarray(M, dtype=float).reshape(9))
        d.vrplanet, d.apix_cm2 = float(vrplanet), float(apix_cm2)
        d.quantity = self._quantity(quantity)
        d.downcast_f32 = int(bool(downcast_f32))
        xe, ze = _f64(xedges), _f64(zedges)
        d.nx, d.nz = len(xe)-1, len(ze)-1
        d.xedges, d.zedges = _p(xe), _p(ze)
        keep = [xe, ze]
        if d.quantity == 1:
            self._fill_lines(d, g_tables, keep)
        self._check(self.lib.nxc_set_image(self._h, C.byref(d)))
        self.image_shape = (int(d.nx), int(d.nz))
        self.ages_owner.pop('image', None)          # the set switches the age block off

    def set_bounce(self, cfg):
        """cfg: dict from nexoclom_amd.surface.bounce_config, or None for perfect sticking.
        ``temp_dependent`` is the sticking law (0 constant, 1 temperature, 2 surface map); with
        ``stick_map`` = (longitude nodes, latitude nodes or None, coefficients) the map is set
        first, so that a refused map leaves the description as it was."""
        if cfg is None:
            self._check(self.lib.nxc_set_bounce(self._h, None))
            return
        if cfg.get('stick_map') is not None:
            self.set_stick_map(*cfg['stick_map'])
        d = nxc_bounce_desc()
        d.GM, d.unit_km = cfg['GM'], cfg['unit_km']
        d.accomfactor, d.stickcoef = cfg['accomfactor'], cfg['stickcoef']
        d.A = (C.c_double*3)(*cfg['A'])
        d.t0, d.t1 = cfg['t0'], cfg['t1']
        d.temp_dependent = int(cfg['temp_dependent'])
        tx, ty, coef = _f64(cfg['tx']), _f64(cfg['ty']), _f64(cfg['coef'])
        d.nx, d.ny = len(tx), len(ty)
        d.tx, d.ty, d.coef = _p(tx), _p(ty), _p(coef)
        d.seed = int(cfg['seed']) & 0xffffffffffffffff
        self._check(self.lib.nxc_set_bounce(self._h, C.byref(d)))

    def set_stick_map(self, longitude, latitude=None, coef=None):
        """The surface map of sticking law 2 (nxc_set_stick_map): coef[nlon, nlat] on the nodes
        ``longitude``, ``latitude`` [rad], or coef[nlon] with ``latitude`` None; ``longitude``
        None clears the map."""
        if longitude is None:
            self._check(self.lib.nxc_set_stick_map(self._h, None))
            return
        lon, val = _f64(longitude), _f64(coef)
        lat = None if latitude is None else _f64(latitude)
        shape = (len(lon),) if lat is None else (len(lon), len(lat))
        if val.shape != shape:
            raise ValueError(f'stick_map: coef{val.shape} does not fit its axes {shape}')
        d = nxc_stick_map_desc()
        d.nlon, d.nlat = len(lon), 0 if lat is None else len(lat)
        d.lon, d.coef = _p(lon), _p(val)
        if lat is not None:
            d.lat = _p(lat)
        self._check(self.lib.nxc_set_stick_map(self._h, C.byref(d)))

    def set_bodies(self, cfg):
        """cfg: dict(moons=[dict(gm, radius, a, omega, phi), ...], t0, chx=dict(k0, rho0, width,
        height, omega)|None) in model units (R, s), or None to clear.  Extension beyond the
        reference (include/nexoclom_hip.h, nxc_bodies_desc)."""
        if cfg is None:
            self._check(self.lib.nxc_set_bodies(self._h, None))
            return
        d = nxc_bodies_desc()
        moons = cfg.get('moons', [])
        if len(moons) > 4:
            raise HipError('at most 4 moons')
        d.n_moons = len(moons)
        for m, mo in enumerate(moons):
            d.gm[m], d.radius[m], d.a[m] = mo['gm'], mo['radius'], mo['a']
            d.omega[m], d.phi[m] = mo['omega'], mo['phi']
        d.t0 = cfg['t0']
        chx = cfg.get('chx')
        d.chx_on = int(chx is not None)
        if chx is not None:
            d.chx_k0, d.chx_rho0, d.chx_width = chx['k0'], chx['rho0'], chx['width']
            d.chx_height, d.chx_omega = chx['height'], chx.get('omega', 0.0)
        self._check(self.lib.nxc_set_bodies(self._h, C.byref(d)))

    def set_first_index(self, first_index):
        self._check(self.lib.nxc_set_first_index(self._h, first_index))

    # -- a-2 / a-1 --------------------------------------------------------------------------
    def state(self, x, y, z, vy):
        x, y, z, vy = map(_f64, (x, y, z, vy))
        n = len(x)
        out = [np.empty(n) for _ in range(4)]
        self._check(self.lib.nxc_state(self._h, n, *[_p(a) for a in (x, y, z, vy, *out)]))
        return np.stack(out[:3], axis=1), out[3]

    def rk5_step(self, X0, h, want_delta=False):
        """X0 (N,8) as the reference's rk5 takes it; returns ((N,8) result, (N,8) delta|None)."""
        X0 = np.asarray(X0, dtype=np.float64)
        n = X0.shape[0]
        soa = _f64(X0.T)
        hh = _f64(np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)))
        out = np.empty((8, n))
        delta = np.empty((8, n)) if want_delta else None
        self._check(self.lib.nxc_rk5_step(self._h, n, _p(soa), _p(hh), _p(out),
                                          _p(delta) if want_delta else None))
        return np.ascontiguousarray(out.T), (np.ascontiguousarray(delta.T) if want_delta else None)

    # -- resident data ----------------------------------------------------------------------
    def upload_packets(self, X0):
        """X0 (N,8) row-major or an (8,N) SoA array flagged by ``soa=True`` via upload_soa."""
        X0 = np.asarray(X0, dtype=np.float64)
        return self.upload_soa(_f64(X0.T))

    def upload_soa(self, soa):
        soa = _f64(soa)
        assert soa.ndim == 2 and soa.shape[0] == 8
        self._check(self.lib.nxc_packets_upload(self._h, soa.shape[1], _p(soa)))
        self.n_packets = soa.shape[1]

    def upload_soa_pieces(self, pieces):
        """The resident set = the (8, n_p) arrays of ``pieces`` one after the other, copied
        column by column from where they are (no concatenated host copy)."""
        pieces = [_f64(p) for p in pieces]
        assert all(p.ndim == 2 and p.shape[0] == 8 for p in pieces)
        counts = (C.c_int64*len(pieces))(*[p.shape[1] for p in pieces])
        ptrs = (_dp*len(pieces))(*[_p(p) for p in pieces])
        self._check(self.lib.nxc_packets_upload_pieces(self._h, len(pieces), counts, ptrs))
        self.n_packets = int(sum(p.shape[1] for p in pieces))

    def sample_packets(self, n, seed, first_index=0, download=False, speed_table=None,
                       surface_map=None, pcg64=None, piece=None, map_nodes=None, map_cdf=None,
                       thermal_spline=None, node_speed_table=None, node_altitude_table=None,
                       node_azimuth_table=None, **src):
        """Draw n initial states on the device (nxc_packets_sample).  ``src``: the scalar fields
        of nxc_source_desc except seed/first_index; ``speed_table`` = (cdf, speeds [km/s]) for
        speed_type 2; ``surface_map`` = density array [nlon, nlat] for spatial_type 1 (see
        Output.source_desc); ``map_nodes`` / ``map_cdf`` = node values [nlon, nlat] and cumulated
        cell masses for spatial_type 2 (with map_lon0, map_lon1, map_s0, map_s1 among ``src``), the
        longitude grid and its cdf for spatial_type 3; ``thermal_spline`` = (tx, ty, coef[nx-4,
        ny-4]) of the v(T, p) spline for speed_type 3 (with t0, t1 among ``src``);
        ``node_speed_table`` = (cdf[nlon * nlat, nv], speeds[nv] [km/s]) for speed_type 4,
        ``node_altitude_table`` / ``node_azimuth_table`` = (cdf[nlon * nlat, n], axis[n] [rad]) for
        angular_type 2: one cdf row per node of ``map_nodes`` (spatial_type 2), lon-major.
        ``pcg64 = (npackets, row0)``: the reference's own seeded stream --
        rows row0 .. row0 + n - 1 of the npackets-long vectors default_rng(seed) would draw.
        ``piece = (offset, total)``: the n packets are part of a resident set of ``total`` that
        several calls fill in ascending order."""
        d = nxc_source_desc()
        for k, v in src.items():
            setattr(d, k, v)
        d.seed = int(seed) & 0xffffffffffffffff
        d.first_index = int(first_index)
        if pcg64 is not None:
            d.generator, d.pcg_n, d.pcg_row0 = 1, int(pcg64[0]), int(pcg64[1])
            d.pcg_state, d.pcg_inc = pcg64_words(seed)
        if piece is not None:
            d.dest_offset, d.dest_total = int(piece[0]), int(piece[1])
        keep = []
        if speed_table is not None:
            cdf, speeds = _f64(speed_table[0]), _f64(speed_table[1])
            if cdf.shape != speeds.shape or cdf.ndim != 1:
                raise ValueError('speed_table must be two 1-D arrays of equal length')
            keep += [cdf, speeds]
            d.n_speed, d.speed_cdf, d.speed_v = len(cdf), _p(cdf), _p(speeds)
        if surface_map is not None:
            dens = _f64(surface_map)
            keep.append(dens)
            d.map_nlon, d.map_nlat, d.map = dens.shape[0], dens.shape[1], _p(dens)
        if map_nodes is not None or map_cdf is not None:
            if surface_map is not None or map_nodes is None or map_cdf is None:
                raise ValueError('a surface map source takes map_nodes and map_cdf, and no '
                                 'surface_map')
            nodes, cdf = _f64(map_nodes), _f64(map_cdf)
            cells = (nodes.shape[0] - 1)*(nodes.shape[1] - 1) if nodes.ndim == 2 else len(nodes)
            if nodes.ndim not in (1, 2) or cdf.ndim != 1 or len(cdf) != cells:
                raise ValueError('map_cdf must hold one entry per cell of map_nodes (2-D) or per '
                                 'node (1-D)')
            keep += [nodes, cdf]
            d.map_nlon, d.map_nlat = nodes.shape[0], nodes.shape[1] if nodes.ndim == 2 else 0
            d.map, d.map_cdf = _p(nodes), _p(cdf)
        if thermal_spline is not None:
            tx, ty, coef = (_f64(a) for a in thermal_spline)
            if tx.ndim != 1 or ty.ndim != 1 or coef.shape != (len(tx) - 4, len(ty) - 4):
                raise ValueError('thermal_spline must be (tx, ty, coef) with coef of shape '
                                 '(len(tx) - 4, len(ty) - 4)')
            keep += [tx, ty, coef]
            d.nx, d.ny, d.tx, d.ty, d.coef = len(tx), len(ty), _p(tx), _p(ty), _p(coef)
        for name, table in (('speed', node_speed_table), ('alt', node_altitude_table),
                            ('az', node_azimuth_table)):
            if table is None:
                continue
            cdf, axis = _f64(table[0]), _f64(table[1])
            if map_nodes is None or cdf.ndim != 2 or axis.ndim != 1 or \
                    cdf.shape != (np.size(map_nodes), len(axis)):
                raise ValueError(f'node_{name} table must be (cdf[nodes, n], axis[n]) with one row '
                                 'per node of map_nodes')
            keep += [cdf, axis]
            setattr(d, f'n_node_{name}', len(axis))
            setattr(d, f'node_{name}_cdf', _p(cdf))
            setattr(d, 'node_speed_v' if name == 'speed' else f'node_{name}', _p(axis))
        n = int(n)
        out = np.empty((8, n)) if download else None
        self._check(self.lib.nxc_packets_sample(self._h, C.byref(d), n,
                                                _p(out) if download else None))
        self.n_packets = n if piece is None else int(piece[1])
        return out

    def image_clear(self):
        self._check(self.lib.nxc_image_clear(self._h))
        self.ages_owner.pop('image', None)          # zeroed with the image

    def image_download(self):
        nx, nz = self.image_shape
        image = np.empty((nx, nz))
        counts = np.empty((nx, nz), dtype=np.uint64)
        self._check(self.lib.nxc_image_download(self._h, _p(image), counts.ctypes.data_as(_u64p)))
        return image, counts

    def counters(self):
        c = nxc_counters()
        self._check(self.lib.nxc_counters_get(self._h, C.byref(c)))
        return {k: int(getattr(c, k)) for k, _ in nxc_counters._fields_ if k != 'wave_trips'}

    def wave_trips(self):
        """Trips of a wave through the persistent step loop in the last integrate call: a
        measurement (it depends on how the lanes happened to be refilled), kept out of
        ``counters()`` -- whose entries are results and repeat exactly."""
        c = nxc_counters()
        self._check(self.lib.nxc_counters_get(self._h, C.byref(c)))
        return int(c.wave_trips)

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(self.lib.nxc_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    # -- a-3 / a-4 --------------------------------------------------------------------------
    def integrate_const(self, step, n_iter, outeredge, image=False, nrec=0, want_final=False,
                        want_steps=False):
        """Constant-step driver over the resident packets.

        nrec > 0 returns the trajectory as an (8, nrec, N) array (lock-step kernel); otherwise the
        persistent lane-refill kernel runs.  Returns dict(traj, final (N,8), steps)."""
        n = self.n_packets
        traj = np.empty((8, nrec, n)) if nrec else None
        final = np.empty((8, n)) if want_final else None
        steps = np.empty(n, dtype=np.int64) if want_steps else None
        self._check(self.lib.nxc_integrate_const(
            self._h, step, n_iter, outeredge, NXC_RUN_IMAGE if image else 0,
            _p(traj) if nrec else None, nrec, _p(final) if want_final else None,
            steps.ctypes.data_as(_i64p) if want_steps else None))
        return dict(traj=traj, final=None if final is None else np.ascontiguousarray(final.T),
                    steps=steps)

    def integrate_const_rows(self, step, n_iter, outeredge, narrow=False, resident=False):
        """Trajectories as Output.save() keeps them: only the records with frac > 0,
        packet-major.  Returns dict(lengths (N,) int64, rows (9, total): the 8 state columns and
        lossfrac); narrow=True delivers them as float32 (save()'s down-cast, done on the device).
        resident=True leaves them in HBM instead: dict(lengths, store: RowStore)."""
        n = self.n_packets
        lengths = np.empty(n, dtype=np.int64)
        total = C.c_int64(0)
        self._check(self.lib.nxc_integrate_const_rows(
            self._h, step, n_iter, outeredge, lengths.ctypes.data_as(_i64p), C.byref(total)))
        if resident:
            # records on their way (10 slots) + the columns that stay (9 + index)
            self.make_room(int(total.value) * 20 * (4 if narrow else 8))
            handle = C.c_void_p()
            self._check(self.lib.nxc_rows_build(self._h, int(narrow), C.byref(handle)))
            store = RowStore(self, handle)
            self._stores.append(weakref.ref(store))
            return dict(lengths=lengths, store=store)
        rows = np.empty((9, int(total.value)), dtype=np.float32 if narrow else np.float64)
        if narrow:
            self._check(self.lib.nxc_rows_fetch_f32(
                self._h, rows.ctypes.data_as(_fp) if total.value else None))
        else:
            self._check(self.lib.nxc_rows_fetch(self._h, _p(rows) if total.value else None))
        return dict(lengths=lengths, rows=rows)

    def integrate_const_async(self, step, n_iter, outeredge, image=True):
        self._check(self.lib.nxc_integrate_const_async(self._h, step, n_iter, outeredge,
                                                       NXC_RUN_IMAGE if image else 0))

    def integrate_const_streamed(self, soa, step, n_iter, outeredge, image=True, pieces=16):
        """Upload the (8, N) host array and integrate it in one pipelined pass (the next piece
        crosses PCIe while the current one is integrated).  Asynchronous: ``synchronize()`` before
        touching ``soa`` or reading results -- it raises HipError (code NXC_ERR_INCOMPLETE) when
        the kernel gave up waiting for its queue, in which case nothing of the pass is valid."""
        soa = _f64(soa)
        assert soa.ndim == 2 and soa.shape[0] == 8
        self._keep = soa                      # the copies read it until the stream is drained
        self._check(self.lib.nxc_integrate_const_streamed(
            self._h, soa.shape[1], _p(soa), pieces, step, n_iter, outeredge,
            NXC_RUN_IMAGE if image else 0))
        self.n_packets = soa.shape[1]

    def integrate_var(self, resolution, outeredge, max_steps=10**6, resident=False):
        """Adaptive-step driver over the resident packets: (final (N, 8), stored step (N,)).
        resident=True leaves the finals in HBM for ``var_rows_build`` and returns the steps only."""
        n = self.n_packets
        hs = np.empty(n)
        if resident:
            self._check(self.lib.nxc_integrate_var_resident(self._h, resolution, outeredge,
                                                            max_steps, _p(hs)))
            return hs
        final = np.empty((8, n))
        self._check(self.lib.nxc_integrate_var(self._h, resolution, outeredge, max_steps,
                                               _p(final), _p(hs)))
        return np.ascontiguousarray(final.T), hs

    def var_rows_build(self, narrow=False, compress=True):
        """The row store of the last ``integrate_var(resident=True)``: one row per kept packet
        (compress: fp64 frac > 0; else all), float32 / int32 when narrow.  Returns (RowStore,
        kept (N,) bool)."""
        n = self.n_packets
        self.make_room(n * 10 * (4 if narrow else 8))
        handle = C.c_void_p()
        kept = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.nxc_var_rows_build(
            self._h, int(bool(narrow)), int(bool(compress)), C.byref(handle),
            kept.ctypes.data_as(_u8p)))
        store = RowStore(self, handle)
        self._stores.append(weakref.ref(store))
        return store, kept.view(np.bool_)

    # -- stored samples: host columns or a RowStore's rows ----------------------------------
    @staticmethod
    def _columns(cols):
        """(entry suffix, ctypes pointers, arrays to keep alive) of host sample columns: float32
        ones (an Output as save() keeps it) go to the device as they are and are widened there
        (suffix '_f32'); anything else is taken as float64 (suffix '')."""
        if all(getattr(c, 'dtype', None) == np.float32 for c in cols):
            cols = [np.ascontiguousarray(c) for c in cols]
            return '_f32', [c.ctypes.data_as(_fp) for c in cols], cols
        cols = [_f64(c) for c in cols]
        return '', [_p(c) for c in cols], cols

    @staticmethod
    def _rows_handle(store):
        """The nxc_rows of a RowStore that is still in HBM."""
        if store._r is None:
            raise HipError('the row store has been freed')
        return store._r

    def _accumulate(self, entry_name, cols, rows):
        """One consumer's pass over stored samples: ``rows = (RowStore, first, count)`` through
        its ``_rows`` entry, else host columns through the entry of their width."""
        if entry_name.endswith('_ages_accumulate'):
            self.ages_owner.pop(entry_name.split('_')[1], None)
        if rows is not None:
            store, first, count = rows
            self._check(getattr(self.lib, entry_name + '_rows')(
                self._h, self._rows_handle(store), first, count))
            return
        suffix, ptrs, cols = self._columns(cols)
        self._check(getattr(self.lib, entry_name + suffix)(self._h, len(cols[0]), *ptrs))

    # -- moon-centred frame: stored rows moved into the frame that co-rotates with a moon -----
    @staticmethod
    def frame_desc(frame):
        """The nxc_frame_desc of ``frame``: one as it is, else built from the attributes omega
        [rad/s], M [R], U [R/s] and scale (a frames.MoonFrame)."""
        if isinstance(frame, nxc_frame_desc):
            return frame
        desc = nxc_frame_desc()
        desc.omega, desc.scale = float(frame.omega), float(frame.scale)
        desc.M[:], desc.U[:] = [float(v) for v in frame.M], [float(v) for v in frame.U]
        return desc

    def frame_rows(self, frame, store, first=0, count=None):
        """Rows [first, first + count) of a RowStore moved into ``frame``: a new RowStore of
        ``count`` rows of the same width, which the caller frees.  It is not entered among the
        stores ``make_room`` may spill: nobody owns its rows."""
        count = store.total - first if count is None else int(count)
        handle = C.c_void_p()
        self._check(self.lib.nxc_frame_rows(self._h, C.byref(self.frame_desc(frame)),
                                            self._rows_handle(store), first, count,
                                            C.byref(handle)))
        return RowStore(self, handle)

    def frame_columns(self, frame, t, x, y, z, vx, vy, vz):
        """Host columns moved into ``frame``: (6, p) x', y', z', vx', vy', vz', float32 when all
        seven columns are (they go over as they are, are widened on the device and rounded
        once), else float64."""
        suffix, ptrs, cols = self._columns((t, x, y, z, vx, vy, vz))
        p = len(cols[0])
        if any(len(c) != p for c in cols):
            raise ValueError('frame_columns: the columns differ in length')
        out = np.empty((6, p), dtype=np.float32 if suffix else np.float64)
        self._check(getattr(self.lib, 'nxc_frame_columns' + suffix)(
            self._h, C.byref(self.frame_desc(frame)), p, *ptrs,
            out.ctypes.data_as(_fp if suffix else _dp)))
        return out

    def frame_columns_f32(self, frame, t, x, y, z, vx, vy, vz):
        """``frame_columns`` of float32 columns (anything else is narrowed first)."""
        return self.frame_columns(frame, *(np.asarray(c, dtype=np.float32)
                                           for c in (t, x, y, z, vx, vy, vz)))

    # a pixel image's velocity products; ``prefix``: 'image' or 'camera', as in nxc_<prefix>_...
    def _moments_enable(self, prefix, on):
        self._check(getattr(self.lib, f'nxc_{prefix}_moments_enable')(self._h, int(bool(on))))

    def _cube_enable(self, prefix, nv, v_lo, v_hi):
        nv = int(nv)
        self._check(getattr(self.lib, f'nxc_{prefix}_cube_enable')(self._h, nv, v_lo, v_hi))
        setattr(self, f'_{prefix}_cube_nv', nv)

    def _ages_enable(self, prefix, na, t0, a_lo, a_hi):
        na = int(na)
        self._check(getattr(self.lib, f'nxc_{prefix}_ages_enable')(self._h, na, t0, a_lo, a_hi))
        setattr(self, f'_{prefix}_ages_na', na)
        self.ages_owner.pop(prefix, None)

    def _block_shape(self, prefix):
        """(sets, records) of a block of sums: ((), the grid's shape), or for the shell map its two
        planes and ``_shell_records()``"""
        if prefix == 'shell':
            return (2,), self._shell_records()
        return (), tuple(getattr(self, prefix + '_shape', None) or (0, 0))

    def _ages_upload(self, prefix, sums):
        sets, records = self._block_shape(prefix)
        shape = sets + records + (getattr(self, f'_{prefix}_ages_na', 0) + 2, 2)
        sums = _f64(sums)
        if sums.shape != shape:
            raise ValueError(f'ages_upload: sums of shape {sums.shape}, the block has {shape}')
        self.ages_owner.pop(prefix, None)
        self._check(getattr(self.lib, f'nxc_{prefix}_ages_upload')(self._h, _p(sums)))

    def _ages_apply(self, prefix, K):
        K = _f64(K)
        if K.ndim != 2 or K.shape[0] != getattr(self, f'_{prefix}_ages_na', 0) + 2:
            raise ValueError('ages_apply: K must have one row per plane, (na + 2, ne)')
        ne = K.shape[1]
        sets, records = self._block_shape(prefix)
        out = np.zeros(sets + (ne,) + records + (2,))
        self._check(getattr(self.lib, f'nxc_{prefix}_ages_apply')(self._h, ne, _p(K), _p(out)))
        return out

    def ages_transient(self, prefix, token, setup, sums, K):
        """The device's part of a product's ``transient()``.  Unless the resident ``prefix`` block
        is the total of the object that holds ``token``, it is seated again: ``setup(self)`` sets
        up and enables, ``sums()`` is uploaded and the owner recorded.  Returns the block
        contracted with ``K`` (``<prefix>_ages_apply``)."""
        if self.ages_owner.get(prefix) is not token:
            setup(self)
            getattr(self, prefix + '_ages_upload')(sums())
            self.ages_owner[prefix] = token
        return getattr(self, prefix + '_ages_apply')(K)

    def _pixel_sums_download(self, prefix, what):
        bins = {'cube': f'_{prefix}_cube_nv', 'ages': f'_{prefix}_ages_na'}
        per_pixel = (4,) if what == 'moments' else (getattr(self, bins[what], 0) + 2, 2)
        sets, records = self._block_shape(prefix)
        sums = np.zeros(sets + records + per_pixel)
        self._check(getattr(self.lib, f'nxc_{prefix}_{what}_download')(self._h, _p(sums)))
        return sums

    QUANTITIES = {'column': 0, 'density': 0, 'radiance': 1, 'difrad': 1}

    @classmethod
    def _quantity(cls, name, allowed=QUANTITIES):
        """nxc_image_desc.quantity / nxc_camera_desc.quantity of a quantity's name"""
        if name not in allowed:
            raise ValueError(f'{name} is invalid.')
        return cls.QUANTITIES[name]

    @staticmethod
    def _fill_lines(desc, g_tables, keep):
        """The g-value tables [(velocities, g)] into a descriptor's line_n / line_v / line_g;
        ``keep`` collects the arrays the descriptor then points into."""
        if len(g_tables) > NXC_MAX_LINES:
            raise ValueError('too many emission lines')
        desc.n_lines = len(g_tables)
        for k, (v, g) in enumerate(g_tables):
            v, g = _f64(v), _f64(g)
            keep += [v, g]
            desc.line_n[k], desc.line_v[k], desc.line_g[k] = len(v), _p(v), _p(g)

    # -- a-6..a-8 ---------------------------------------------------------------------------
    def image_accumulate(self, x, y, z, vy, frac):
        """Bin stored samples given as host columns (float32 ones go over as they are)."""
        self._accumulate('nxc_image_accumulate', (x, y, z, vy, frac), None)

    IMAGE_MODES = {'auto': 0, 'atomics': 1, 'tiles': 2}

    def image_mode(self, mode='auto', tile_pixels=0, slab_samples=0):
        """How stored samples reach the image: 'atomics' (one global atomic pair per binned
        sample), 'tiles' (filed by image tile, summed in LDS, handed over once per pixel), or
        'auto' (tiles from 2^17 samples on).  Packet counts are identical either way."""
        self._check(self.lib.nxc_image_mode(self._h, self.IMAGE_MODES.get(mode, mode),
                                            tile_pixels, slab_samples))

    def image_accumulate_rows(self, store, first=0, count=None):
        """Bin rows [first, first + count) of a RowStore: no host round trip."""
        count = store.total - first if count is None else int(count)
        self._accumulate('nxc_image_accumulate', None, (store, first, count))

    def image_moments_enable(self, on=True):
        """After ``set_image``: allocate and zero the four velocity-moment sums per pixel (``on``
        false frees them; the next ``set_image`` switches them off)."""
        self._moments_enable('image', on)

    def image_moments_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                 frac=None, rows=None):
        """Add samples to the image pair and to the pixel moments in one pass (always the atomic
        path): seven host columns (float32 ones go over as they are), or ``rows = (RowStore,
        first, count)``."""
        self._accumulate('nxc_image_moments_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def image_moments_download(self):
        """(nx, nz, 4) float64: the sums m1 m2 m3 ww of every pixel (PIXEL_MOMENT_COLUMNS)."""
        return self._pixel_sums_download('image', 'moments')

    def image_cube_enable(self, nv, v_lo=0.0, v_hi=0.0):
        """After ``set_image``: allocate and zero a velocity cube of ``nv`` bins over [v_lo, v_hi)
        [R/s] beside the image pair (``nv`` 0 frees it; the next ``set_image`` switches it off)."""
        self._cube_enable('image', nv, v_lo, v_hi)

    def image_cube_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                              frac=None, rows=None):
        """Add samples to the image pair and to its velocity cube in one pass: seven host columns (float32
        ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_image_cube_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def image_cube_download(self):
        """(nx, nz, nv + 2, 2) float64: {sum w, sum w w} per pixel and plane -- plane 0 below the
        range, 1..nv the bins, nv + 1 at or above it (or not a number)."""
        return self._pixel_sums_download('image', 'cube')

    def image_ages_enable(self, na, t0=0.0, a_lo=0.0, a_hi=0.0):
        """After ``set_image``: allocate and zero an age block of ``na`` bins over [a_lo, a_hi) [s]
        for rows read at the epoch ``t0`` [s] beside the image pair (``na`` 0 frees it; the next
        ``set_image`` switches it off)."""
        self._ages_enable('image', na, t0, a_lo, a_hi)

    def image_ages_accumulate(self, time=None, x=None, y=None, z=None, vy=None, frac=None,
                              rows=None):
        """Add samples to the image pair and to its age block in one pass: six host columns, the
        time first (float32 ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_image_ages_accumulate', (time, x, y, z, vy, frac), rows)

    def image_ages_download(self):
        """(nx, nz, na + 2, 2) float64: {sum w, sum w w} per pixel and plane -- plane 0 younger
        than the range, 1..na the bins, na + 1 at or above it (or a time that is not a number)."""
        return self._pixel_sums_download('image', 'ages')

    def image_ages_upload(self, sums):
        """Replace the resident age block by ``sums`` (nx, nz, na + 2, 2)."""
        self._ages_upload('image', sums)

    def image_ages_apply(self, K):
        """The resident age block contracted with ``K`` (na + 2, ne): (ne, nx, nz, 2) float64,
        {sum_k S K, sum_k WW K K} per epoch and pixel, summed over the planes in their order."""
        return self._ages_apply('image', K)

    # -- f-1: spacecraft lines of sight ------------------------------------------------------
    def los_accumulate(self, dphi, sin_dphi, sin_2dphi, cos_threshold, vrplanet, unit_cm, g_tables,
                       ladder, sc, x=None, y=None, z=None, vy=None, frac=None, index=None,
                       n_index=0, used_cap=0, rows=None, pairs=None, vx=None, vz=None,
                       profile=False, ages=False, time=None):
        """sc: (8, S) array x,y,z,xbore,ybore,zbore,dist_from_plan,ladder_len.  Samples: five host
        columns (+ index), or ``rows = (RowStore, first, count, index_shift)`` for rows that are
        already in HBM.  Returns dict(radiance, npackets, included|None, used (2, m)|None,
        n_used).  ``pairs``: a PairList that receives the used pairs on the device instead of
        ``used`` (HipError with code NXC_ERR_OVERFLOW when they do not fit).  ``profile``: the
        pass also adds to the profile of ``los_profile_enable``; host columns then come with
        ``vx`` and ``vz`` (a row store carries them).  ``ages``: the pass also adds to the block of
        ``los_ages_enable``; host columns then come with ``time`` (a row store carries it).  One
        pass does one of the two."""
        if profile and ages:
            raise ValueError('profile=True and ages=True exclude each other: one pass does one')
        if profile and rows is None and (vx is None or vz is None):
            raise ValueError('profile=True over host columns needs vx and vz')
        if ages and rows is None and time is None:
            raise ValueError('ages=True over host columns needs time')
        if pairs is not None and used_cap:
            raise ValueError('used_cap and pairs exclude each other')
        name = ('nxc_los_profile_accumulate' if profile else
                'nxc_los_ages_accumulate' if ages else 'nxc_los_accumulate')
        d, keep = self._los_desc(dphi, sin_dphi, sin_2dphi, cos_threshold, vrplanet, unit_cm,
                                 g_tables, ladder)
        sc = _f64(sc)
        S = sc.shape[1]
        if rows is not None:
            store, first, count, shift = rows
            entry = getattr(self.lib, name + '_rows')
            samples = (self._rows_handle(store), first, count, shift)
        else:
            suffix, ptrs, cols = self._columns((x, y, z, vx, vy, vz, frac) if profile else
                                               (time, x, y, z, vy, frac) if ages else
                                               (x, y, z, vy, frac))
            idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64)
            entry = getattr(self.lib, name + suffix)
            samples = (len(cols[0]), *ptrs, idx.ctypes.data_as(_i64p) if idx is not None else None)
        radiance = np.zeros(S)
        npackets = np.zeros(S, dtype=np.int64)
        included = np.zeros(n_index, dtype=np.uint8) if n_index else None
        used = np.zeros((2, used_cap), dtype=np.int64) if used_cap else None
        n_used = C.c_int64(0)
        if pairs is not None:          # the pass writes its used pairs there, not to ``used``
            self._check(self.lib.nxc_los_set_pairs(self._h, pairs._p))
        try:
            self._check(entry(
                self._h, C.byref(d), S, _p(sc), *samples, n_index, _p(radiance),
                npackets.ctypes.data_as(_i64p),
                included.ctypes.data_as(_u8p) if included is not None else None,
                used_cap, used.ctypes.data_as(_i64p) if used is not None else None,
                C.byref(n_used)))
        finally:
            if pairs is not None:
                self.lib.nxc_los_set_pairs(self._h, None)
        m = min(int(n_used.value), used_cap)
        return dict(radiance=radiance, npackets=npackets,
                    included=None if included is None else included.astype(bool),
                    used=None if used is None else used[:, :m], n_used=int(n_used.value))

    def los_profile_enable(self, S, nv, v_lo=0.0, v_hi=0.0):
        """Allocate and zero the line-of-sight profile of ``S`` spectra: ``nv`` bins over
        [v_lo, v_hi) [R/s] and four moment sums per spectrum (``nv`` 0 frees it; a second enable
        replaces and zeroes it)."""
        S, nv = int(S), int(nv)
        self._check(self.lib.nxc_los_profile_enable(self._h, S, nv, v_lo, v_hi))
        self._los_profile_shape = (S, nv) if nv else None

    def los_profile_download(self):
        """(sums (S, nv + 2, 2), moments (S, 4)) float64: {sum w, sum w w} per spectrum and
        record -- record 0 below the range, 1..nv the bins, nv + 1 at or above it (or not a
        number) -- and the sums m1 m2 m3 ww (PIXEL_MOMENT_COLUMNS) of every spectrum."""
        S, nv = getattr(self, '_los_profile_shape', None) or (0, 0)
        sums, moments = np.zeros((S, nv + 2, 2)), np.zeros((S, 4))
        self._check(self.lib.nxc_los_profile_download(self._h, _p(sums), _p(moments)))
        return sums, moments

    def los_ages_enable(self, S, na, t0=0.0, a_lo=0.0, a_hi=0.0):
        """Allocate and zero the line-of-sight ages of ``S`` spectra: ``na`` bins over
        [a_lo, a_hi) seconds of age at the epoch ``t0`` (``na`` 0 frees them; a second enable
        replaces and zeroes them)."""
        S, na = int(S), int(na)
        self._check(self.lib.nxc_los_ages_enable(self._h, S, na, t0, a_lo, a_hi))
        self._los_ages_shape = (S, na) if na else None

    def los_ages_download(self):
        """sums (S, na + 2, 2) float64: {sum w, sum w w} per spectrum and plane -- plane 0 younger
        than the range, 1..na the bins, na + 1 at or above it (or a time that is not a number)."""
        S, na = getattr(self, '_los_ages_shape', None) or (0, 0)
        sums = np.zeros((S, na + 2, 2))
        self._check(self.lib.nxc_los_ages_download(self._h, _p(sums)))
        return sums

    @staticmethod
    def _los_desc(dphi, sin_dphi, sin_2dphi, cos_threshold, vrplanet, unit_cm, g_tables, ladder):
        """(nxc_los_desc, the arrays it points into)"""
        d = nxc_los_desc()
        d.dphi, d.sin_dphi, d.sin_2dphi, d.cos_threshold = dphi, sin_dphi, sin_2dphi, cos_threshold
        d.vrplanet, d.unit_cm = float(vrplanet), float(unit_cm)
        keep = []
        Context._fill_lines(d, g_tables, keep)
        lad = _f64(ladder)
        keep.append(lad)
        d.n_ladder, d.ladder = len(lad), _p(lad)
        return d, keep

    # -- ModelDensity -----------------------------------------------------------------------
    def density_set(self, points, cell_start, origin, h, dr, dims):
        """Upload a query-point index (ModelDensity.DensityIndex: points (Q, 3) sorted by cell,
        int32 cell starts, grid origin, cell edge h and dims) and zero the per-point sums."""
        pts = _f64(points).reshape(-1, 3)
        starts = np.ascontiguousarray(cell_start, dtype=np.int32)
        d = nxc_density_desc()
        d.origin[:] = [float(v) for v in origin]
        d.h, d.dr = float(h), float(dr)
        d.dims[:] = [int(v) for v in dims]
        d.n_points = len(pts)
        d.points = _p(pts) if len(pts) else None
        d.cell_start = starts.ctypes.data_as(_i32p)
        self._check(self.lib.nxc_density_set(self._h, C.byref(d)))
        self._density_q = len(pts)
        self._density_spectrum_nv = 0            # the set switches the spectrum off
        self.density_shape = (len(pts),)         # what the age block's helpers call the pixels
        self._density_ages_na = 0                # ... and the age block
        self.ages_owner.pop('density', None)

    def density_accumulate(self, x=None, y=None, z=None, frac=None, rows=None):
        """Add samples to the per-point sums: four host columns (float32 ones go over as they
        are and are widened on the device), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_density_accumulate', (x, y, z, frac), rows)

    def density_download(self):
        """(frac sums, counts) per indexed point, float64, in the index's point order."""
        q = getattr(self, '_density_q', 0)
        total, count = np.zeros(q), np.zeros(q)
        self._check(self.lib.nxc_density_download(self._h, _p(total), _p(count)))
        return total, count

    def density_moments_enable(self, on=True):
        """After ``density_set``: allocate and zero the ten velocity-moment sums per indexed point
        (``on`` false switches them off; so does the next ``density_set``)."""
        self._check(self.lib.nxc_density_moments_enable(self._h, int(bool(on))))

    def density_moments_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                   frac=None, rows=None):
        """Add samples to the per-point {frac sum, count} and to the moment sums in one pass: seven
        host columns (float32 ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_density_moments_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def density_moments_download(self):
        """(Q, 10) float64 in the index's point order: the sums of f v_a (x, y, z), of
        (f v_a) v_b (xx, yy, zz, xy, xz, yz) and of f f over the samples within dr."""
        sums = np.zeros((getattr(self, '_density_q', 0), 10))
        self._check(self.lib.nxc_density_moments_download(self._h, _p(sums)))
        return sums

    def density_spectrum_enable(self, nv, s_lo=0.0, s_hi=0.0, cos_half=-1.0, all_sky=True,
                                frames=None):
        """After ``density_set``: allocate and zero a spectrum of ``nv`` speed bins over
        [s_lo, s_hi) [R/s] per indexed point, seen through a cone of half angle acos(cos_half)
        (``all_sky``: no cone), and upload ``frames`` (Q, 8) = ux uy uz 0 bx by bz 0 in the index's
        point order (``nv = 0`` frees the spectrum; the next ``density_set`` switches it off)."""
        nv = int(nv)
        if nv == 0:
            self._check(self.lib.nxc_density_spectrum_enable(self._h, None))
            self._density_spectrum_nv = 0
            return
        fr = _f64(np.zeros((getattr(self, '_density_q', 0), 8)) if frames is None else frames)
        if fr.ndim != 2 or fr.shape[1] != 8:
            raise ValueError('frames must have the shape (Q, 8)')
        d = nxc_density_spectrum_desc()
        d.nv, d.s_lo, d.s_hi, d.cos_half = nv, float(s_lo), float(s_hi), float(cos_half)
        d.all_sky = int(bool(all_sky))
        # the library compares the number of records with the points of its own index
        d.n_frames = len(fr)
        d.frames = _p(fr) if len(fr) else None
        self._check(self.lib.nxc_density_spectrum_enable(self._h, C.byref(d)))
        self._density_spectrum_nv = nv

    def density_spectrum_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                    frac=None, rows=None):
        """Add samples to the per-point {frac sum, count} and to the spectrum in one pass: seven
        host columns (float32 ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_density_spectrum_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def density_spectrum_download(self):
        """(2, Q, nv + 2, 2) float64, the device's own order: plane 0 sums f, plane 1 f s, per
        indexed point and speed plane (0 below, 1..nv the bins, nv + 1 above), {sum, sum of
        squares} over the seen samples within dr."""
        nv = getattr(self, '_density_spectrum_nv', 0)
        sums = np.zeros((2, getattr(self, '_density_q', 0), nv + 2, 2))
        self._check(self.lib.nxc_density_spectrum_download(self._h, _p(sums)))
        return sums

    def density_ages_enable(self, na, t0=0.0, a_lo=0.0, a_hi=0.0):
        """After ``density_set``: allocate and zero an age block of ``na`` bins over [a_lo, a_hi)
        seconds of age at the epoch ``t0`` [s] per indexed point (``na = 0`` frees it; the next
        ``density_set`` switches it off)."""
        self._ages_enable('density', na, t0, a_lo, a_hi)

    def density_ages_accumulate(self, time=None, x=None, y=None, z=None, frac=None, rows=None):
        """Add samples to the per-point {frac sum, count} and to the age block in one pass: five
        host columns, time first (float32 ones go over as they are), or ``rows = (RowStore, first,
        count)``."""
        self._accumulate('nxc_density_ages_accumulate', (time, x, y, z, frac), rows)

    def density_ages_download(self):
        """(Q, na + 2, 2) float64 in the index's point order: {sum f, sum f f} per age plane (0
        below, 1..na the bins, na + 1 above) over the samples within dr."""
        return self._pixel_sums_download('density', 'ages')

    def density_ages_upload(self, sums):
        """Replace the age block by ``sums`` (Q, na + 2, 2), in the index's point order."""
        self._ages_upload('density', sums)

    def density_ages_apply(self, K):
        """(ne, Q, 2) = the resident age block contracted with ``K`` (na + 2, ne), as
        ``image_ages_apply`` does it for pixels."""
        return self._ages_apply('density', K)

    # -- CameraImage ------------------------------------------------------------------------
    def camera_set(self, observer, basis, vrplanet, pix_area_cm2, quantity, uedges, vedges,
                   g_tables=()):
        """Describe a pinhole camera (nxc_camera_desc) and zero its resident image: position
        ``observer`` [R], ``basis`` (3, 3) with rows right, boresight, up, tangent-plane bin edges
        and ``pix_area_cm2`` = du dv unit_cm^2."""
        d = nxc_camera_desc()
        d.o = (C.c_double*3)(*np.asarray(observer, dtype=float).reshape(3))
        d.C = (C.c_double*9)(*np.asarray(basis, dtype=float).reshape(9))
        d.vrplanet, d.pix_area_cm2 = float(vrplanet), float(pix_area_cm2)
        d.quantity = self._quantity(quantity, ('column', 'radiance'))
        ue, ve = _f64(uedges), _f64(vedges)
        d.nx, d.nz = len(ue)-1, len(ve)-1
        d.uedges, d.vedges = _p(ue), _p(ve)
        keep = [ue, ve]
        if d.quantity == 1:
            self._fill_lines(d, g_tables, keep)
        self._check(self.lib.nxc_camera_set(self._h, C.byref(d)))
        self.camera_shape = (int(d.nx), int(d.nz))
        self.ages_owner.pop('camera', None)         # the set switches the age block off

    def camera_accumulate(self, x=None, y=None, z=None, vy=None, frac=None, rows=None):
        """Add samples to the camera image: five host columns (float32 ones go over as they are
        and are widened on the device), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_camera_accumulate', (x, y, z, vy, frac), rows)

    def camera_download(self):
        """(image (nx, nz) float64, packet counts (nx, nz) uint64) of the camera."""
        shape = getattr(self, 'camera_shape', None) or (0, 0)
        image = np.zeros(shape)
        counts = np.zeros(shape, dtype=np.uint64)
        self._check(self.lib.nxc_camera_download(
            self._h, _p(image), counts.ctypes.data_as(_u64p)))
        return image, counts

    def camera_moments_enable(self, on=True):
        """After ``camera_set``: allocate and zero the four velocity-moment sums per pixel of the
        camera image (``on`` false frees them; the next ``camera_set`` switches them off)."""
        self._moments_enable('camera', on)

    def camera_moments_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                  frac=None, rows=None):
        """Add samples to the camera image and to its pixel moments in one pass: seven host
        columns, or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_camera_moments_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def camera_moments_download(self):
        """(nx, nz, 4) float64: the sums m1 m2 m3 ww of every pixel of the camera image."""
        return self._pixel_sums_download('camera', 'moments')

    def camera_cube_enable(self, nv, v_lo=0.0, v_hi=0.0):
        """After ``camera_set``: allocate and zero a velocity cube of ``nv`` bins over [v_lo, v_hi)
        [R/s] beside the camera image (``nv`` 0 frees it; the next ``camera_set`` switches it off)."""
        self._cube_enable('camera', nv, v_lo, v_hi)

    def camera_cube_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                               frac=None, rows=None):
        """Add samples to the camera image and to its velocity cube in one pass: seven host columns (float32
        ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_camera_cube_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def camera_cube_download(self):
        """(nx, nz, nv + 2, 2) float64: {sum w, sum w w} per pixel and plane -- plane 0 below the
        range, 1..nv the bins, nv + 1 at or above it (or not a number)."""
        return self._pixel_sums_download('camera', 'cube')

    def camera_ages_enable(self, na, t0=0.0, a_lo=0.0, a_hi=0.0):
        """After ``camera_set``: allocate and zero an age block of ``na`` bins over [a_lo, a_hi) [s]
        for rows read at the epoch ``t0`` [s] beside the camera image (``na`` 0 frees it; the next
        ``camera_set`` switches it off)."""
        self._ages_enable('camera', na, t0, a_lo, a_hi)

    def camera_ages_accumulate(self, time=None, x=None, y=None, z=None, vy=None, frac=None,
                              rows=None):
        """Add samples to the camera image and to its age block in one pass: six host columns, the
        time first (float32 ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_camera_ages_accumulate', (time, x, y, z, vy, frac), rows)

    def camera_ages_download(self):
        """(nx, nz, na + 2, 2) float64: {sum w, sum w w} per pixel and plane -- plane 0 younger
        than the range, 1..na the bins, na + 1 at or above it (or a time that is not a number)."""
        return self._pixel_sums_download('camera', 'ages')

    def camera_ages_upload(self, sums):
        """Replace the resident age block by ``sums`` (nx, nz, na + 2, 2)."""
        self._ages_upload('camera', sums)

    def camera_ages_apply(self, K):
        """The resident age block contracted with ``K`` (na + 2, ne): (ne, nx, nz, 2) float64,
        {sum_k S K, sum_k WW K K} per epoch and pixel, summed over the planes in their order."""
        return self._ages_apply('camera', K)

    # -- ShellMap ---------------------------------------------------------------------------
    def shell_set(self, vrplanet, quantity, lon_edges, mu_edges, r_lo, r_hi, nalt, g_tables=()):
        """Describe a shell map (nxc_shell_desc) and zero its resident sums: longitude edges
        np.linspace(0, 2 pi, nlon + 1), sin(latitude) edges np.linspace(-1, 1, nlat + 1) and
        ``nalt`` altitude bins over [r_lo, r_hi) [R from the centre]."""
        d = nxc_shell_desc()
        d.vrplanet, d.r_lo, d.r_hi = float(vrplanet), float(r_lo), float(r_hi)
        d.quantity = self._quantity(quantity, ('column', 'radiance'))
        le, me = _f64(lon_edges), _f64(mu_edges)
        d.nlon, d.nlat, d.nalt = len(le)-1, len(me)-1, int(nalt)
        d.lon_edges, d.mu_edges = _p(le), _p(me)
        keep = [le, me]
        if d.quantity == 1:
            self._fill_lines(d, g_tables, keep)
        self._check(self.lib.nxc_shell_set(self._h, C.byref(d)))
        self.shell_shape = (int(d.nlon), int(d.nlat), int(d.nalt))
        self._shell_ages_na = 0                  # the set switches the age block off
        self.ages_owner.pop('shell', None)

    def shell_accumulate(self, x=None, y=None, z=None, vy=None, frac=None, rows=None):
        """Add samples to the shell map: five host columns (float32 ones go over as they are and
        are widened on the device), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_shell_accumulate', (x, y, z, vy, frac), rows)

    def shell_download(self):
        """(column (nlon, nlat) float64, packet counts (nlon, nlat) uint64, sums (2, nlon, nlat,
        nalt + 2, 2) float64: {sum w, sum w w} and {sum c, sum c c}, c = w / r^2, per cell and
        altitude record -- record 0 below r_lo, 1..nalt the bins, nalt + 1 at or above r_hi)."""
        nlon, nlat, nalt = getattr(self, 'shell_shape', None) or (0, 0, 0)
        column = np.zeros((nlon, nlat))
        counts = np.zeros((nlon, nlat), dtype=np.uint64)
        sums = np.zeros((2, nlon, nlat, nalt + 2, 2))
        self._check(self.lib.nxc_shell_download(
            self._h, _p(column), counts.ctypes.data_as(_u64p), _p(sums)))
        return column, counts, sums

    def shell_moments_enable(self, on=True):
        """After ``shell_set``: allocate and zero the six planes of velocity sums per cell and
        altitude record (``on`` false frees them; the next ``shell_set`` switches them off)."""
        self._check(self.lib.nxc_shell_moments_enable(self._h, int(bool(on))))

    def shell_moments_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                 frac=None, rows=None):
        """Add samples to the shell map and to its velocity sums in one pass: seven host columns
        (float32 ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_shell_moments_accumulate', (x, y, z, vx, vy, vz, frac), rows)

    def shell_moments_download(self):
        """(6, nlon, nlat, nalt + 2, 2) float64: the twelve sums of ShellMap.SHELL_MOMENT_COLUMNS
        per cell and altitude record, plane by plane (include/nexoclom_hip.h, "ShellMap moments")."""
        nlon, nlat, nalt = getattr(self, 'shell_shape', None) or (0, 0, 0)
        sums = np.zeros((6, nlon, nlat, nalt + 2, 2))
        self._check(self.lib.nxc_shell_moments_download(self._h, _p(sums)))
        return sums

    def _shell_records(self):
        nlon, nlat, nalt = getattr(self, 'shell_shape', None) or (0, 0, 0)
        return (nlon, nlat, nalt + 2 if nlon else 0)

    def shell_ages_enable(self, na, t0=0.0, a_lo=0.0, a_hi=0.0):
        """After ``shell_set``: allocate and zero an age block of ``na`` bins over [a_lo, a_hi)
        seconds of age at the epoch ``t0`` [s] per cell and altitude record, two planes (``na = 0``
        frees it; the next ``shell_set`` switches it off)."""
        self._ages_enable('shell', na, t0, a_lo, a_hi)

    def shell_ages_accumulate(self, time=None, x=None, y=None, z=None, vy=None, frac=None,
                              rows=None):
        """Add samples to the shell map and to its age block in one pass: six host columns, time
        first (float32 ones go over as they are), or ``rows = (RowStore, first, count)``."""
        self._accumulate('nxc_shell_ages_accumulate', (time, x, y, z, vy, frac), rows)

    def shell_ages_download(self):
        """(2, nlon, nlat, nalt + 2, na + 2, 2) float64: {sum w, sum w w} and {sum c, sum c c},
        c = w / r^2, per cell, altitude record and age plane (0 below, 1..na the bins, na + 1
        above; include/nexoclom_hip.h, "ShellMap ages")."""
        return self._pixel_sums_download('shell', 'ages')

    def shell_ages_upload(self, sums):
        """Replace the age block by ``sums`` (2, nlon, nlat, nalt + 2, na + 2, 2)."""
        self._ages_upload('shell', sums)

    def shell_ages_apply(self, K):
        """(2, ne, nlon, nlat, nalt + 2, 2) = both planes of the resident age block contracted
        with ``K`` (na + 2, ne), as ``image_ages_apply`` does it for pixels: {sum_k S K,
        sum_k WW K K} per epoch and record, summed over the age planes in their order."""
        return self._ages_apply('shell', K)

    # -- LOSResultFitted ----------------------------------------------------------------------
    def pairs_create(self, capacity):
        return PairList(self, capacity)

    def fit_set(self, position, ratio, mask, weight_mode=None, weight=None):
        """Per spectrum: spacecraft position (3, S), ratio = data / unfitted model, mask, and for
        weight_mode 'sigma' the weight 1/sigma*2; zeroes the fitted radiance sums."""
        pos = _f64(position).reshape(3, -1)
        S = pos.shape[1]
        ratio = _f64(ratio)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if len(ratio) != S or len(mask) != S:
            raise ValueError('position, ratio and mask must describe the same spectra')
        d = nxc_fit_desc()
        d.n_spectra, d.weight_mode = S, FIT_WEIGHT_MODES[weight_mode]
        d.position, d.ratio = _p(pos), _p(ratio)
        w = None
        if weight_mode == 'sigma':
            w = _f64(weight)
            d.weight = _p(w)
        d.mask = mask.ctypes.data_as(_u8p)
        self._check(self.lib.nxc_fit_set(self._h, C.byref(d)))
        self._fit_s = S

    def fit_source(self, x=None, y=None, z=None, vy=None, frac=None, index=None, rows=None):
        """The samples the pairs' rows index: five host columns with their packet index (float32
        ones go over as they are), or ``rows = (RowStore, first, count, index_shift)``."""
        if rows is not None:
            store, first, count, shift = rows
            r = self._rows_handle(store)
            self._fit_store = store
            self._check(self.lib.nxc_fit_source_rows(self._h, r, first, count, shift))
            return
        self._fit_store = None
        suffix, ptrs, cols = self._columns((x, y, z, vy, frac))
        idx = np.ascontiguousarray(index, dtype=np.int64)
        self._check(getattr(self.lib, 'nxc_fit_source' + suffix)(
            self._h, len(idx), *ptrs, idx.ctypes.data_as(_i64p)))

    def fit_packets(self, pairs, n_packets):
        """Per packet num, den, cnt and the multiplier mult over ``pairs`` (a PairList) and the
        source; also the sum of f and the number of packets seen.  The multipliers stay on the
        device for fit_radiance / fit_rows."""
        n = int(n_packets)
        num, den, mult = np.zeros(n), np.zeros(n), np.zeros(n)
        cnt = np.zeros(n, dtype=np.int32)
        stats = np.zeros(2)
        self._check(self.lib.nxc_fit_packets(self._h, pairs._p, n, _p(num), _p(den),
                                             cnt.ctypes.data_as(_i32p), _p(mult), _p(stats)))
        return dict(num=num, den=den, cnt=cnt, mult=mult, f_sum=float(stats[0]),
                    n_seen=int(stats[1]))

    def fit_radiance(self, pairs, dphi, sin_dphi, vrplanet, unit_cm, g_tables):
        """Add the fitted radiance of every pair to its spectrum's sum (Apix with ``dphi``)."""
        d, keep = self._los_desc(dphi, sin_dphi, 0.0, 0.0, vrplanet, unit_cm, g_tables, [0.0])
        self._check(self.lib.nxc_fit_radiance(self._h, pairs._p, C.byref(d)))

    def fit_rows(self, n_packets, compress=True):
        """(RowStore of the fitted rows, rows kept per packet) for a row-store source."""
        lengths = np.zeros(int(n_packets), dtype=np.int64)
        handle = C.c_void_p()
        self._check(self.lib.nxc_fit_rows(self._h, int(bool(compress)), C.byref(handle),
                                          lengths.ctypes.data_as(_i64p)))
        store = RowStore(self, handle)
        self._stores.append(weakref.ref(store))
        return store, lengths

    def fit_download(self):
        out = np.zeros(getattr(self, '_fit_s', 0))
        self._check(self.lib.nxc_fit_download(self._h, _p(out)))
        return out

    # -- source maps ------------------------------------------------------------------------
    def source_map_set(self, grid):
        """Upload a source-map grid (sourcemap.SourceMapGrid: edges, point centres, cos and
        thresholds per latitude row, tile segments) and zero the resident map."""
        keep = [_f64(a) for a in (grid.alt_edges, grid.az_edges, grid.lon_edges, grid.lat_edges,
                                  grid.lon, grid.lat, grid.cos_lat, grid.threshold)]
        seg = np.ascontiguousarray(grid.seg, dtype=np.int32).reshape(-1, 2)
        seg_off = np.ascontiguousarray(grid.seg_off, dtype=np.int32)
        d = nxc_source_map_desc()
        d.nlon, d.nlat, d.nvel, d.nalt, d.naz = (int(v) for v in (
            grid.nlon, grid.nlat, grid.nvel, grid.nalt, grid.naz))
        d.tile, d.r_km = int(grid.tile), float(grid.r_km)
        (d.alt_edges, d.az_edges, d.lon_edges, d.lat_edges, d.point_lon, d.point_lat,
         d.point_cos, d.threshold) = (_p(a) for a in keep)
        d.n_seg = len(seg)
        d.seg = seg.ctypes.data_as(_i32p) if len(seg) else None
        d.seg_off = seg_off.ctypes.data_as(_i32p)
        self._check(self.lib.nxc_source_map_set(self._h, C.byref(d)))
        self._smap = (int(grid.nlon)*int(grid.nlat), int(grid.nvel), int(grid.nalt), int(grid.naz))

    def source_map_accumulate(self, lat, lon, v, alt, az, frac, cell_start, vel_edges,
                              available, factor):
        """Add one Output's packets (sorted by cell) to the resident map, its speed histograms
        times ``factor``.  Returns the Output's whole-planet speed, altitude and azimuth histograms
        and its speed map summed over the grid."""
        _, nvel, nalt, naz = self._smap
        cols = [_f64(c) for c in (lat, lon, v, alt, az, frac)]
        starts = np.ascontiguousarray(cell_start, dtype=np.int32)
        edges = _f64(vel_edges)
        small = np.zeros(nvel + nalt + naz + nvel)
        n = len(cols[0])
        if any(len(c) != n for c in cols) or len(starts) != self._smap[0] + 1 or \
                len(edges) != nvel + 1:
            raise ValueError('source_map_accumulate: column, cell-start or edge lengths differ '
                             'from the grid')
        ptr = [(_p(c) if n else None) for c in cols]
        self._check(self.lib.nxc_source_map_accumulate(
            self._h, n, *ptr, starts.ctypes.data_as(_i32p), _p(edges),
            int(bool(available)), factor, _p(small)))
        return dict(speed_dist=small[:nvel], altitude_dist=small[nvel:nvel + nalt],
                    azimuth_dist=small[nvel + nalt:nvel + nalt + naz],
                    speed_gridsum=small[nvel + nalt + naz:])

    def source_map_download(self):
        """(map [npoints, nvel + nalt + naz + 3], unsmeared histogram [npoints])."""
        npoints, nvel, nalt, naz = self._smap
        out = np.zeros((npoints, nvel + nalt + naz + 3))
        hist2d = np.zeros(npoints)
        self._check(self.lib.nxc_source_map_download(self._h, _p(out), _p(hist2d)))
        return out, hist2d

    # -- RCCL -------------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_uint8*NXC_UNIQUE_ID_BYTES)()
        self._check(self.lib.nxc_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_uint8*NXC_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self.lib.nxc_comm_init(self._h, buf, rank, nranks))

    def comm_destroy(self):
        self._check(self.lib.nxc_comm_destroy(self._h))

    def image_allreduce(self):
        self._check(self.lib.nxc_image_allreduce(self._h))

    def allreduce_max(self, value):
        v = C.c_double(value)
        self._check(self.lib.nxc_allreduce_max_f64(self._h, C.byref(v)))
        return float(v.value)

    def allreduce_sum(self, value):
        v = C.c_double(value)
        self._check(self.lib.nxc_allreduce_sum_f64(self._h, C.byref(v)))
        return float(v.value)

    def barrier(self):
        self._check(self.lib.nxc_barrier(self._h))

    def allreduce(self, values):
        """Sum over the ranks of a small float64 array (returned; LOSResult.py:264-266 across
        GPUs)."""
        v = np.array(values, dtype=np.float64).ravel()
        self._check(self.lib.nxc_allreduce_f64(self._h, _p(v), v.size))
        return v.reshape(np.shape(values))

    def comm_set_timeout(self, seconds):
        """Deadline of every wait on a collective (default 120 s): past it the communicator is
        aborted and the waiting call raises HipError (code NXC_ERR_RCCL)."""
        self._check(self.lib.nxc_comm_set_timeout(self._h, seconds))

    def comm_abort(self):
        self._check(self.lib.nxc_comm_abort(self._h))

    def comm_request_abort(self):
        """Thread-safe: ends the owning thread's wait on a collective (or its next collective)
        with HipError instead of letting it run to the deadline."""
        if self._h:
            self.lib.nxc_comm_request_abort(self._h)

    def comm_test_stall(self, seconds):
        """Fault injection: the stream is busy for ``seconds`` as if a collective hung."""
        self._check(self.lib.nxc_comm_test_stall(self._h, seconds))

    # -- measurement helpers ----------------------------------------------------------------
    def stream_copy_gbs(self, nbytes=1 << 31, reps=5):
        """The box's streaming-copy rate, GB/s of bytes read + written."""
        gbs = C.c_double(0)
        self._check(self.lib.nxc_stream_copy_gbs(self._h, nbytes, reps, C.byref(gbs)))
        return float(gbs.value)

    def shader_clock_mhz(self):
        """The shader clock the chip holds under an fp64 load (in-kernel stamps)."""
        mhz = C.c_double(0)
        self._check(self.lib.nxc_shader_clock_mhz(self._h, C.byref(mhz)))
        return float(mhz.value)

    # -- diagnostics ------------------------------------------------------------------------
    def pcg64_uniforms(self, seed, n, row0, count, nvec):
        """(nvec, count): rows row0.. of the first nvec ``default_rng(seed).random(n)`` vectors,
        as the device sampler's generator 1 forms them."""
        state, inc = pcg64_words(seed)
        out = np.empty((nvec, count))
        self._check(self.lib.nxc_pcg64_uniforms(self._h, state, inc, n, row0, count, nvec, _p(out)))
        return out

    def math(self, which, x, y=None):
        code = {'exp': 0, 'log': 1, 'cube': 2, 'sqrt': 3, 'div': 4}[which]
        x = _f64(x)
        out = np.empty_like(x)
        y2 = _f64(y) if y is not None else None
        self._check(self.lib.nxc_math_batch(self._h, code, len(x), _p(x),
                                            _p(y2) if y2 is not None else None, _p(out)))
        return out
