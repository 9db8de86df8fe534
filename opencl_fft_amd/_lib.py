"""ctypes binding of libclfft_amd.so (the C ABI in include/clfft_amd.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``make -C opencl_fft_amd/csrc``.  There is no fallback: if the library is
missing, or it finds no HIP device, the error is raised to the caller.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CLFA_LIB_PATH: another build of the same library, for A/B runs of bench.py — tools/build_variant.sh)
LIB_PATH = os.environ.get("CLFA_LIB_PATH") or os.path.join(_HERE, "libclfft_amd.so")
if os.environ.get("CLFA_LIB_PATH"):   # a development hook: never silently (bench.py also records the path in its line)
    import sys
    print("opencl_fft_amd: CLFA_LIB_PATH is set, loading %s instead of the in-tree library" % LIB_PATH, file=sys.stderr)

# every symbol include/clfft_amd.h declares: (name, restype, argtypes)
_vp, _fp, _ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
SYMBOLS = [
    ("clfa_device_count", C.c_int, [_ip]),
    ("clfa_device_name", C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    ("clfa_error_string", C.c_char_p, [C.c_int]),
    ("clfa_version", C.c_char_p, []),
    ("clfa_bitrev_table", C.c_int, [C.c_int, _ip]),
    ("clfa_twiddle_table", C.c_int, [C.c_int, C.c_int, _fp]),
    ("clfa_r2c_twiddle_table", C.c_int, [C.c_int, C.c_int, _fp]),
    ("clfa_cfft_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int]),
    ("clfa_rfft_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int]),
    ("clfa_fft_destroy", None, [_vp]),
    ("clfa_fft_get_error", C.c_int, [_vp]),
    ("clfa_fft_get_log", C.c_char_p, [_vp]),
    ("clfa_cfft_transform", C.c_int, [_vp, _vp, C.c_long]),
    ("clfa_rfft_transform", C.c_int, [_vp, _vp, _vp, C.c_long]),
    ("clfa_fft_host_alloc", C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    ("clfa_fft_host_free", C.c_int, [_vp, _vp]),
    ("clfa_fft_exec_dev", C.c_int, [_vp, _vp, C.c_long, _vp]),
    ("clfa_fft_exec_dev_oop", C.c_int, [_vp, _vp, _vp, C.c_long, _vp]),
    ("clfa_fft_device_buffers", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    ("clfa_fft_run_buffers", C.c_int, [_vp]),
    ("clfa_fft_device_tables", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("clfa_copy_to_device", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int]),
    ("clfa_copy_from_device", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int]),
    ("clfa_stream_synchronize", C.c_int, [_vp]),
    ("clfa_fft_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_fft_kernel_name", C.c_char_p, [_vp]),
    ("clfa_fft_balance_record", C.c_int, [_vp, C.c_int]),
    ("clfa_fft_balance_read", C.c_int, [_vp, _vp, C.c_int, _ip]),
    ("clfa_fft_balance_counters", C.c_int, [_vp, _vp, C.c_int, _ip]),
    ("clfa_reorder_dev", C.c_int, [C.c_int, _vp, _vp, C.c_int, C.c_long, _vp]),
    ("clfa_pconv_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int]),
    ("clfa_pconv_destroy", None, [_vp]),
    ("clfa_pconv_get_error", C.c_int, [_vp]),
    ("clfa_pconv_nparts", C.c_int, [_vp]),
    ("clfa_pconv_wp", C.c_int, [_vp]),
    ("clfa_pconv_wp2", C.c_int, [_vp]),
    ("clfa_pconv_push_ir", C.c_int, [_vp, _vp]),
    ("clfa_pconv_push_ir_dev", C.c_int, [_vp, _vp, C.c_long, _vp]),
    ("clfa_bandwidth_probe", C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    ("clfa_pconv_convolution", C.c_int, [_vp, _vp, _vp]),
    ("clfa_pconv_convolution_tv", C.c_int, [_vp, _vp, _vp, _vp]),
    ("clfa_pconv_process_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("clfa_pconv_state_bytes", C.c_size_t, [_vp]),
    ("clfa_pconv_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pconv_process_blocks_dev", C.c_int, [_vp, _vp, C.c_long, _vp, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_pconv_convolution_blocks", C.c_int, [_vp, _vp, _vp, _vp, C.c_long]),
    ("clfa_pconv_blocks_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_pconv_blocks_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pconv_matrix_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("clfa_pconv_matrix_destroy", None, [_vp]),
    ("clfa_pconv_matrix_get_error", C.c_int, [_vp]),
    ("clfa_pconv_matrix_get_log", C.c_char_p, [_vp]),
    ("clfa_pconv_matrix_push_ir", C.c_int, [_vp, _vp]),
    ("clfa_pconv_matrix_push_ir_dev", C.c_int, [_vp, _vp, C.c_long, _vp]),
    ("clfa_pconv_matrix_push_ir_fade", C.c_int, [_vp, _vp, C.c_long]),
    ("clfa_pconv_matrix_push_ir_fade_dev", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_pconv_matrix_fade_remaining", C.c_long, [_vp]),
    ("clfa_pconv_matrix_process_dev", C.c_int, [_vp, _vp, C.c_long, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_pconv_matrix_convolution", C.c_int, [_vp, _vp, _vp, C.c_long]),
    ("clfa_pconv_matrix_nparts", C.c_int, [_vp]),
    ("clfa_pconv_matrix_state_bytes", C.c_size_t, [_vp]),
    ("clfa_pconv_matrix_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_pconv_matrix_kernel_name", C.c_char_p, [_vp]),
    ("clfa_nupconv_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("clfa_nupconv_destroy", None, [_vp]),
    ("clfa_nupconv_get_error", C.c_int, [_vp]),
    ("clfa_nupconv_get_log", C.c_char_p, [_vp]),
    ("clfa_nupconv_nparts", C.c_int, [_vp, C.c_int]),
    ("clfa_nupconv_position", C.c_long, [_vp]),
    ("clfa_nupconv_state_bytes", C.c_size_t, [_vp]),
    ("clfa_nupconv_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_nupconv_kernel_name", C.c_char_p, [_vp]),
    ("clfa_nupconv_push_ir", C.c_int, [_vp, _vp]),
    ("clfa_nupconv_push_ir_dev", C.c_int, [_vp, _vp, C.c_long, _vp]),
    ("clfa_nupconv_push_ir_fade", C.c_int, [_vp, _vp, C.c_long]),
    ("clfa_nupconv_push_ir_fade_dev", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_nupconv_fade_remaining", C.c_long, [_vp]),
    ("clfa_nupconv_process_dev", C.c_int, [_vp, _vp, C.c_long, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_nupconv_convolution", C.c_int, [_vp, _vp, _vp, C.c_long]),
    ("clfa_nupconv_process_tv_dev", C.c_int, [_vp, _vp, C.c_long, _vp, C.c_long, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_nupconv_convolution_tv", C.c_int, [_vp, _vp, _vp, _vp, C.c_long]),
    ("clfa_nupconv_tv_period", C.c_long, [_vp]),
    ("clfa_nupconv_reset", C.c_int, [_vp, _vp]),
    ("clfa_nupconv_matrix_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("clfa_nupconv_matrix_destroy", None, [_vp]),
    ("clfa_nupconv_matrix_get_error", C.c_int, [_vp]),
    ("clfa_nupconv_matrix_get_log", C.c_char_p, [_vp]),
    ("clfa_nupconv_matrix_nparts", C.c_int, [_vp, C.c_int]),
    ("clfa_nupconv_matrix_segments", C.c_int, [_vp, C.c_int]),
    ("clfa_nupconv_matrix_position", C.c_long, [_vp]),
    ("clfa_nupconv_matrix_state_bytes", C.c_size_t, [_vp]),
    ("clfa_nupconv_matrix_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_nupconv_matrix_kernel_name", C.c_char_p, [_vp]),
    ("clfa_nupconv_matrix_push_ir", C.c_int, [_vp, _vp]),
    ("clfa_nupconv_matrix_push_ir_dev", C.c_int, [_vp, _vp, C.c_long, _vp]),
    ("clfa_nupconv_matrix_push_ir_fade", C.c_int, [_vp, _vp, C.c_long]),
    ("clfa_nupconv_matrix_push_ir_fade_dev", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_nupconv_matrix_fade_remaining", C.c_long, [_vp]),
    ("clfa_nupconv_matrix_process_dev",C.c_int, [_vp, _vp, C.c_long, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_nupconv_matrix_convolution", C.c_int, [_vp, _vp, _vp, C.c_long]),
    ("clfa_nupconv_matrix_reset", C.c_int, [_vp, _vp]),
    ("clfa_dconv_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int]),
    ("clfa_dconv_destroy", None, [_vp]),
    ("clfa_dconv_get_error", C.c_int, [_vp]),
    ("clfa_dconv_push_ir", C.c_int, [_vp, _vp]),
    ("clfa_dconv_convolution", C.c_int, [_vp, _vp, _vp]),
    ("clfa_dconv_convolution_tv", C.c_int, [_vp, _vp, _vp, _vp]),
    ("clfa_dconv_process_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("clfa_dconv_create_channels", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int]),
    ("clfa_dconv_push_ir_dev", C.c_int, [_vp, _vp, C.c_long, _vp]),
    ("clfa_dconv_process_blocks_dev", C.c_int, [_vp, _vp, C.c_long, _vp, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_dconv_convolution_blocks", C.c_int, [_vp, _vp, _vp, _vp, C.c_long]),
    ("clfa_dconv_channels", C.c_int, [_vp]),
    ("clfa_dconv_wp", C.c_int, [_vp]),
    ("clfa_dconv_state_bytes", C.c_size_t, [_vp]),
    ("clfa_dconv_blocks_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_dconv_blocks_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_stft_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    ("clfa_stft_destroy", None, [_vp]),
    ("clfa_stft_get_error", C.c_int, [_vp]),
    ("clfa_stft_get_log", C.c_char_p, [_vp]),
    ("clfa_stft_frames", C.c_long, [_vp, C.c_long]),
    ("clfa_stft_samples", C.c_long, [_vp, C.c_long]),
    ("clfa_stft_analyze_dev", C.c_int, [_vp, _vp, C.c_long, C.c_long, C.c_long, _vp, _vp]),
    ("clfa_stft_synthesize_dev", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp, C.c_long, C.c_int, _vp]),
    ("clfa_stft_analyze", C.c_int, [_vp, _vp, C.c_long, C.c_long, C.c_long, _vp]),
    ("clfa_stft_synthesize", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp, C.c_long, C.c_int]),
    ("clfa_stft_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_stft_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pvoc_create", C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]),
    ("clfa_pvoc_destroy", None, [_vp]),
    ("clfa_pvoc_get_error", C.c_int, [_vp]),
    ("clfa_pvoc_get_log", C.c_char_p, [_vp]),
    ("clfa_pvoc_reset", C.c_int, [_vp]),
    ("clfa_pvoc_analyze_dev", C.c_int, [_vp, _vp, _vp, C.c_long, _vp]),
    ("clfa_pvoc_synthesize_dev", C.c_int, [_vp, _vp, _vp, C.c_long, _vp]),
    ("clfa_pvoc_analyze", C.c_int, [_vp, _vp, _vp, C.c_long]),
    ("clfa_pvoc_synthesize", C.c_int, [_vp, _vp, _vp, C.c_long]),
    ("clfa_pvoc_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_pvoc_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_pvoc_scan_chunk", C.c_int, []),
    ("clfa_pvoc_read_phase", C.c_int, [_vp, _vp]),
    ("clfa_pvoc_read_prev", C.c_int, [_vp, _vp]),
    ("clfa_pvoc_scale_dev", C.c_int, [_vp, _vp, _vp, C.c_long, _vp, C.c_int, C.c_float, C.c_int, _vp]),
    ("clfa_pvoc_shift_dev", C.c_int, [_vp, _vp, _vp, C.c_long, _vp, C.c_int, C.c_int, C.c_float, C.c_int, _vp]),
    ("clfa_pvoc_read_dev", C.c_int, [_vp, _vp, C.c_long, _vp, _vp, C.c_long, _vp]),
    ("clfa_pvoc_scale", C.c_int, [_vp, _vp, _vp, C.c_long, _vp, C.c_int, C.c_float, C.c_int]),
    ("clfa_pvoc_shift", C.c_int, [_vp, _vp, _vp, C.c_long, _vp, C.c_int, C.c_int, C.c_float, C.c_int]),
    ("clfa_pvoc_read", C.c_int, [_vp, _vp, C.c_long, _vp, _vp, C.c_long]),
    ("clfa_pvoc_ops_kernel_name", C.c_char_p, [_vp, C.c_int, C.c_int]),
    ("clfa_pvoc_tanal_dev", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp, _vp, _vp, C.c_long, _vp]),
    ("clfa_pvoc_tanal", C.c_int, [_vp, _vp, C.c_long, C.c_long, _vp, _vp, _vp, C.c_long]),
    ("clfa_pvoc_tanal_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pvoc_pair_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_long, _vp, _vp, C.c_int, _vp]),
    ("clfa_pvoc_pair", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_long, _vp, _vp, C.c_int]),
    ("clfa_pvoc_pair_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_pvoc_shape_dev", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_long, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    ("clfa_pvoc_shape", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_long, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("clfa_pvoc_shape_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_pvoc_blur_setup", C.c_int, [_vp, C.c_int]),
    ("clfa_pvoc_time_dev", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_long, _vp, _vp, _vp]),
    ("clfa_pvoc_time", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_long, _vp, _vp]),
    ("clfa_pvoc_time_read_state", C.c_int, [_vp, C.c_int, _vp]),
    ("clfa_pvoc_time_state_bytes", C.c_size_t, [_vp]),
    ("clfa_pvoc_blur_max_frames", C.c_int, [_vp]),
    ("clfa_pvoc_time_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_pvoc_delay_setup", C.c_int, [_vp, C.c_int]),
    ("clfa_pvoc_delay_dev", C.c_int, [_vp, _vp, _vp, C.c_long, _vp, _vp, _vp]),
    ("clfa_pvoc_delay", C.c_int, [_vp, _vp, _vp, C.c_long, _vp, _vp]),
    ("clfa_pvoc_delay_read_state", C.c_int, [_vp, C.c_int, _vp]),
    ("clfa_pvoc_delay_state_bytes", C.c_size_t, [_vp]),
    ("clfa_pvoc_delay_max_frames", C.c_int, [_vp]),
    ("clfa_pvoc_delay_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_pvoc_desc_dev", C.c_int, [_vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, _vp]),
    ("clfa_pvoc_desc", C.c_int, [_vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int]),
    ("clfa_pvoc_desc_read_state", C.c_int, [_vp, _vp]),
    ("clfa_pvoc_desc_state_bytes", C.c_size_t, [_vp]),
    ("clfa_pvoc_desc_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pvoc_bank_setup", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("clfa_pvoc_bank_bands", C.c_int, [_vp]),
    ("clfa_pvoc_bank_read_dct", C.c_int, [_vp, _vp]),
    ("clfa_pvoc_bank_state_bytes", C.c_size_t, [_vp]),
    ("clfa_pvoc_bands_dev", C.c_int, [_vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_float, _vp]),
    ("clfa_pvoc_bands", C.c_int, [_vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_float]),
    ("clfa_pvoc_bands_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pvoc_trace_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, _vp]),
    ("clfa_pvoc_trace", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int]),
    ("clfa_pvoc_trace_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pvoc_demix_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, _vp]),
    ("clfa_pvoc_demix", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int]),
    ("clfa_pvoc_demix_kernel_name", C.c_char_p, [_vp, C.c_int]),
    ("clfa_pvoc_pitch_dev", C.c_int, [_vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_float, C.c_float, C.c_float, _vp]),
    ("clfa_pvoc_pitch", C.c_int, [_vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                  C.c_float, C.c_float]),
    ("clfa_pvoc_pitch_kernel_name", C.c_char_p, [_vp]),
    ("clfa_pvoc_adsyn_dev",C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, C.c_int, C.c_int, C.c_float, _vp, C.c_long, _vp]),
    ("clfa_pvoc_adsyn", C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, C.c_int, C.c_int, C.c_float, _vp, C.c_long]),
    ("clfa_pvoc_adsyn_read_state", C.c_int, [_vp, _vp, _vp, _vp]),
    ("clfa_pvoc_adsyn_workspace_bytes", C.c_size_t, [_vp]),
    ("clfa_pvoc_adsyn_tile_bins", C.c_int, []),
    ("clfa_pvoc_adsyn_kernel_name", C.c_char_p, [_vp]),
]

_LIB = None


def _preload_torch_hip():
    """One HIP runtime per process.  The PyTorch-ROCm wheel ships its own
    libamdhip64.so.7 (+ its own HSA runtime) under torch/lib with the same
    soname as /opt/rocm's; the dynamic loader keeps whichever is loaded first,
    and a process that mixes the two loses its GPUs.  Callers use torch for
    device memory and streams, so when torch is installed its runtime is loaded
    first and libclfft_amd.so binds to it (found by spec, torch is not imported)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    """Load libclfft_amd.so once; raises OSError if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C opencl_fft_amd/csrc`" % LIB_PATH)
        _preload_torch_hip()
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)          # AttributeError if the ABI is incomplete
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


class ClError(RuntimeError):
    """An OpenCL-numbered status returned by the library (0 is success)."""

    def __init__(self, code, where=""):
        self.code = code
        msg = lib().clfa_error_string(code).decode()
        super().__init__("%s: %s (%d)" % (where, msg, code) if where else "%s (%d)" % (msg, code))


def check(code, where=""):
    if code != 0:
        raise ClError(code, where)
    return code
