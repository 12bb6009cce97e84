"""ctypes binding of libstofnet_amd.so (the C ABI in include/stofnet_amd.h).

There is no CPU or PyTorch fallback: if the HIP library is missing or a tensor is
not on a ROCm device the call raises.  PyTorch is used only for device memory and
streams.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('STOF_LIB_PATH') or os.path.join(_HERE, 'libstofnet_amd.so')   # override: ablation builds only

STOF_OK = 0
STOF_ERR_BAD_ARG = 1
STOF_ERR_ODD_SGB_REMAINDER = 2
STOF_ERR_UNSUPPORTED = 3
STOF_ERR_WORKSPACE = 4
STOF_ERR_HIP = 5
STOF_ERR_CHANNELS = 6
STOF_ERR_POOL_EMPTY = 7

PREC_FP32 = 0
PREC_F16X3 = 1
NUM_PARAMS = 30


class NetDesc(ctypes.Structure):
    _fields_ = [('upsample_factor', ctypes.c_int32), ('semi_global_scale', ctypes.c_int32),
                ('precision', ctypes.c_int32), ('seg_policy', ctypes.c_int32)]


class ZonziniDesc(ctypes.Structure):
    _fields_ = [('variant', ctypes.c_int32), ('reserved', ctypes.c_int32)]


ZONZINI_SMALL = 0
ZONZINI_LARGE = 1


class SincNetDesc(ctypes.Structure):
    _fields_ = [('fs', ctypes.c_double), ('bn_eps', ctypes.c_double), ('stop_after', ctypes.c_int32),
                ('reserved', ctypes.c_int32)]


class EdsrDesc(ctypes.Structure):
    _fields_ = [('num_blocks', ctypes.c_int32), ('upscale_factor', ctypes.c_int32)]


class EspcnDesc(ctypes.Structure):
    _fields_ = [('upscale_factor', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class WaveUnetDesc(ctypes.Structure):
    _fields_ = [('n_layers', ctypes.c_int32), ('channels_interval', ctypes.c_int32)]


class KuleshovDesc(ctypes.Structure):
    _fields_ = [('input_length', ctypes.c_int64), ('output_length', ctypes.c_int64), ('bn_eps', ctypes.c_double),
                ('tile_variant', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class AugmentDesc(ctypes.Structure):
    _fields_ = [('seed', ctypes.c_uint64), ('crop_ratio', ctypes.c_double), ('snr_db', ctypes.c_double),
                ('normalize', ctypes.c_int32), ('add_noise', ctypes.c_int32), ('rank', ctypes.c_uint32),
                ('call', ctypes.c_uint32)]


class DasDesc(ctypes.Structure):
    _fields_ = [('c', ctypes.c_double), ('t0', ctypes.c_double), ('fs', ctypes.c_double), ('f0', ctypes.c_double),
                ('fnumber', ctypes.c_double), ('dtype', ctypes.c_int32), ('compound', ctypes.c_int32)]


DAS_F32, DAS_F64, DAS_C64, DAS_C128 = 0, 1, 2, 3


class StofnetLibraryMissing(ImportError):
    pass


_c = ctypes
_SIGNATURES = {
    'stof_status_string': (_c.c_char_p, [_c.c_int]),
    'stof_abi_version': (_c.c_int, []),
    'stof_packed_weights_bytes': (_c.c_size_t, [_c.POINTER(NetDesc)]),
    'stof_pack_weights': (_c.c_int, [_c.POINTER(NetDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_forward_workspace_bytes': (_c.c_size_t, [_c.POINTER(NetDesc), _c.c_int64, _c.c_int64]),
    'stof_forward': (_c.c_int, [_c.POINTER(NetDesc), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64,
                                _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_forward_checked': (_c.c_int, [_c.POINTER(NetDesc), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                        _c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    'stof_forward_events': (_c.c_int, [_c.POINTER(NetDesc), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                       _c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.POINTER(_c.c_void_p),
                                       _c.c_void_p]),
    'stof_forward_onsets_workspace_bytes': (_c.c_size_t, [_c.POINTER(NetDesc), _c.c_int64, _c.c_int64]),
    'stof_forward_onsets': (_c.c_int, [_c.POINTER(NetDesc), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64,
                                       _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                       _c.c_void_p]),
    'stof_forward_auto': (_c.c_int, [_c.POINTER(NetDesc), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                     _c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p,
                                     _c.POINTER(_c.c_void_p)]),
    'stof_events_create': (_c.c_int, [_c.c_int32, _c.POINTER(_c.c_void_p)]),
    'stof_events_destroy': (_c.c_int, [_c.c_int32, _c.POINTER(_c.c_void_p)]),
    'stof_event_elapsed_ms': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_float)]),
    'stof_sample_shuffle': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32,
                                       _c.c_void_p]),
    'stof_sample_shuffle_bytes': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32,
                                             _c.c_int32, _c.c_void_p]),
    'stof_pick_maxima': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_float,
                                    _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    'stof_indices_to_coords': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_float,
                                          _c.c_void_p, _c.c_void_p]),
    'stof_reduce_echoes': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64,
                                      _c.c_int64, _c.c_float, _c.c_void_p, _c.c_void_p]),
    'stof_hilbert_workspace_bytes': (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    'stof_hilbert': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_hilbert_f64_workspace_bytes': (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    'stof_hilbert_f64': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_hilbert_streamed': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_gradpeak_moments': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                         _c.c_void_p, _c.c_void_p]),
    'stof_gradpeak_blurred_stride': (_c.c_int64, [_c.c_int64, _c.c_int32]),
    'stof_gradpeak_moments_store': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                               _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_grad_peak_detect_blurred': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_float,
                                                 _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int64, _c.c_void_p, _c.c_int64,
                                                 _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_gradpeak_threshold': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_grad_peak_detect': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                         _c.c_float, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int64, _c.c_void_p,
                                         _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_toa_detect_fused_ok': (_c.c_int, [_c.c_int64, _c.c_int32]),
    'stof_toa_detect': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_float,
                                   _c.c_int32, _c.c_int32, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                   _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_toa_moments': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32, _c.c_void_p,
                                    _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_gradpeak_moments_f64_workspace_bytes': (_c.c_size_t, [_c.c_int64]),
    'stof_gradpeak_moments_f64': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                             _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_gradpeak_threshold_f64': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_grad_peak_detect_f64': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_int32,
                                             _c.c_double, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int64, _c.c_void_p,
                                             _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_zonzini_packed_bytes': (_c.c_size_t, [_c.POINTER(ZonziniDesc)]),
    'stof_zonzini_pack_weights': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_zonzini_workspace_bytes': (_c.c_size_t, [_c.POINTER(ZonziniDesc), _c.c_int64, _c.c_int64]),
    'stof_zonzini_forward': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_zonzini_train_pack': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_zonzini_train_forward': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p,
                                              _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p]),
    'stof_zonzini_train_head_bwd': (_c.c_int, [_c.POINTER(ZonziniDesc)] + [_c.c_void_p] * 10 + [_c.c_int64, _c.c_void_p]),
    'stof_zonzini_train_conv_wgrad_workspace_bytes': (_c.c_size_t, [_c.POINTER(ZonziniDesc), _c.c_int32]),
    'stof_zonzini_train_conv_wgrad': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.c_int32] + [_c.c_void_p] * 5 +
                                      [_c.c_int64, _c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_zonzini_train_dgrad_image_floats': (_c.c_size_t, [_c.POINTER(ZonziniDesc), _c.c_int32]),
    'stof_zonzini_train_dgrad_image': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_zonzini_train_conv_dgrad': (_c.c_int, [_c.POINTER(ZonziniDesc), _c.c_int32] + [_c.c_void_p] * 4 +
                                      [_c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_zonzini_train_in_wgrad_workspace_bytes': (_c.c_size_t, [_c.POINTER(ZonziniDesc)]),
    'stof_zonzini_train_in_wgrad': (_c.c_int, [_c.POINTER(ZonziniDesc)] + [_c.c_void_p] * 5 +
                                    [_c.c_int64, _c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_zonzini_train_in_dgrad': (_c.c_int, [_c.POINTER(ZonziniDesc)] + [_c.c_void_p] * 4 + [_c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_sincnet_packed_bytes': (_c.c_size_t, [_c.POINTER(SincNetDesc)]),
    'stof_sincnet_pack_weights': (_c.c_int, [_c.POINTER(SincNetDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_sincnet_filter_bank': (_c.c_int, [_c.POINTER(SincNetDesc), _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_sincnet_workspace_bytes': (_c.c_size_t, [_c.POINTER(SincNetDesc), _c.c_int64, _c.c_int64]),
    'stof_sincnet_forward': (_c.c_int, [_c.POINTER(SincNetDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_sincnet_band_grad': (_c.c_int, [_c.POINTER(SincNetDesc)] + [_c.c_void_p] * 5),
    'stof_sincnet_train_buffer_floats': (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    'stof_sincnet_train_blob_layout': (_c.c_int, [_c.POINTER(_c.c_int64)]),
    'stof_sincnet_train_pack': (_c.c_int, [_c.POINTER(SincNetDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_sincnet_device_pack': (_c.c_int, [_c.POINTER(SincNetDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_sincnet_train_dgrad_image': (_c.c_int, [_c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_sincnet_train_conv': (_c.c_int, [_c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p]),
    'stof_sincnet_train_conv_dgrad': (_c.c_int, [_c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_sincnet_train_stats_workspace_bytes': (_c.c_size_t, []),
    'stof_sincnet_train_stats': (_c.c_int, [_c.POINTER(SincNetDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32] + [_c.c_void_p] * 4 +
                                 [_c.c_double] + [_c.c_void_p] * 4 + [_c.c_size_t, _c.c_void_p]),
    'stof_sincnet_train_apply': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_sincnet_train_bn_bwd': (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int64, _c.c_int64, _c.c_int32] + [_c.c_void_p] * 4 +
                                  [_c.c_size_t, _c.c_void_p]),
    'stof_sincnet_train_conv_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32]),
    'stof_sincnet_train_conv_wgrad': (_c.c_int, [_c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                                 _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_sincnet_train_out_wgrad_workspace_bytes': (_c.c_size_t, []),
    'stof_sincnet_train_out_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                _c.c_size_t, _c.c_void_p]),
    'stof_sincnet_train_out_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p]),
    'stof_sincnet_train_bank_grad_workspace_bytes': (_c.c_size_t, []),
    'stof_sincnet_train_bank_grad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                _c.c_void_p]),
    'stof_sincnet_train_band_grad': (_c.c_int, [_c.POINTER(SincNetDesc)] + [_c.c_void_p] * 6),
    'stof_sincnet_train_in_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p]),
    'stof_edsr_packed_bytes': (_c.c_size_t, [_c.POINTER(EdsrDesc)]),
    'stof_edsr_pack_weights': (_c.c_int, [_c.POINTER(EdsrDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_edsr_workspace_bytes': (_c.c_size_t, [_c.POINTER(EdsrDesc), _c.c_int64, _c.c_int64]),
    'stof_edsr_forward': (_c.c_int, [_c.POINTER(EdsrDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                     _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_espcn_packed_bytes': (_c.c_size_t, [_c.POINTER(EspcnDesc)]),
    'stof_espcn_pack_weights': (_c.c_int, [_c.POINTER(EspcnDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_espcn_forward': (_c.c_int, [_c.POINTER(EspcnDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                      _c.c_void_p, _c.c_void_p]),
    'stof_waveunet_packed_bytes': (_c.c_size_t, [_c.POINTER(WaveUnetDesc)]),
    'stof_waveunet_pack_weights': (_c.c_int, [_c.POINTER(WaveUnetDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_waveunet_workspace_bytes': (_c.c_size_t, [_c.POINTER(WaveUnetDesc), _c.c_int64, _c.c_int64]),
    'stof_waveunet_forward': (_c.c_int, [_c.POINTER(WaveUnetDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_waveunet_train_constants': (_c.c_int, [_c.POINTER(_c.c_int64)]),
    'stof_waveunet_interp_table': (_c.c_int, [_c.c_int64] + [_c.c_void_p] * 6),
    'stof_waveunet_train_frag_floats': (_c.c_size_t, [_c.c_int32] * 4),
    'stof_waveunet_train_pack_frag': (_c.c_int, [_c.c_void_p] + [_c.c_int32] * 4 + [_c.c_void_p] * 2),
    'stof_waveunet_train_pack_in': (_c.c_int, [_c.c_void_p] * 4),
    'stof_waveunet_train_in_conv': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_waveunet_train_conv': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64] + [_c.c_int32] * 5 + [_c.c_void_p] * 4),
    'stof_waveunet_train_stats_workspace_bytes': (_c.c_size_t, []),
    'stof_waveunet_train_stats': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32] + [_c.c_void_p] * 4 + [_c.c_double] * 2 +
                                  [_c.c_void_p] * 4 + [_c.c_size_t, _c.c_void_p]),
    'stof_waveunet_train_apply': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_waveunet_train_head': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64] + [_c.c_void_p] * 4),
    'stof_waveunet_train_head_bwd_workspace_bytes': (_c.c_size_t, []),
    'stof_waveunet_train_head_bwd': (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int64, _c.c_int64] + [_c.c_void_p] * 6 + [_c.c_size_t, _c.c_void_p]),
    'stof_waveunet_train_bn_bwd': (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int64, _c.c_int32] + [_c.c_void_p] * 4 + [_c.c_size_t, _c.c_void_p]),
    'stof_waveunet_train_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int64, _c.c_int64] + [_c.c_int32] * 3),
    'stof_waveunet_train_wgrad': (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int64, _c.c_int64] + [_c.c_int32] * 5 + [_c.c_void_p] * 3 +
                                  [_c.c_size_t, _c.c_void_p]),
    'stof_waveunet_train_in_wgrad_workspace_bytes': (_c.c_size_t, []),
    'stof_waveunet_train_in_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64] + [_c.c_void_p] * 3 + [_c.c_size_t, _c.c_void_p]),
    'stof_waveunet_train_interp_t': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_void_p]),
    'stof_waveunet_train_skip_sum': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_void_p]),
    'stof_waveunet_train_in_dgrad': (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p]),
    'stof_kuleshov_packed_bytes': (_c.c_size_t, [_c.POINTER(KuleshovDesc)]),
    'stof_kuleshov_pack_weights': (_c.c_int, [_c.POINTER(KuleshovDesc), _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_size_t]),
    'stof_kuleshov_workspace_bytes': (_c.c_size_t, [_c.POINTER(KuleshovDesc), _c.c_int64]),
    'stof_kuleshov_forward': (_c.c_int, [_c.POINTER(KuleshovDesc), _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_kuleshov_dropout_keep': (_c.c_int, [_c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_int32, _c.c_int64, _c.c_int64, _c.c_double,
                                              _c.c_void_p]),
    'stof_kuleshov_train_constants': (_c.c_int, [_c.POINTER(_c.c_int64)]),
    'stof_kuleshov_train_frag_floats': (_c.c_size_t, [_c.c_int32] * 4),
    'stof_kuleshov_train_pack_frag': (_c.c_int, [_c.c_void_p] + [_c.c_int32] * 4 + [_c.c_void_p] * 2),
    'stof_kuleshov_train_pack_final': (_c.c_int, [_c.c_void_p] * 3),
    'stof_kuleshov_train_fc_frag_floats': (_c.c_size_t, [_c.POINTER(KuleshovDesc)]),
    'stof_kuleshov_train_pack_fc': (_c.c_int, [_c.POINTER(KuleshovDesc)] + [_c.c_void_p] * 3),
    'stof_kuleshov_train_down0': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64] + [_c.c_void_p] * 4),
    'stof_kuleshov_train_conv': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64] + [_c.c_int32] * 4 + [_c.c_void_p] * 2 +
                                 [_c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_kuleshov_train_stats_workspace_bytes': (_c.c_size_t, []),
    'stof_kuleshov_train_stats': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int32] + [_c.c_void_p] * 4 + [_c.c_double] * 2 +
                                  [_c.c_void_p] * 4 + [_c.c_size_t, _c.c_void_p]),
    'stof_kuleshov_train_apply_down': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                                  _c.c_void_p]),
    'stof_kuleshov_train_apply_up': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p, _c.c_uint64, _c.c_uint32,
                                                _c.c_uint32, _c.c_int32, _c.c_double, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    'stof_kuleshov_train_apply_bott': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_double,
                                                  _c.c_void_p, _c.c_void_p]),
    'stof_kuleshov_train_tail': (_c.c_int, [_c.POINTER(KuleshovDesc), _c.c_void_p, _c.c_int64] + [_c.c_void_p] * 7),
    'stof_kuleshov_train_fc_bwd': (_c.c_int, [_c.POINTER(KuleshovDesc)] + [_c.c_void_p] * 3 + [_c.c_int64] + [_c.c_void_p] * 4),
    'stof_kuleshov_train_final_bwd_workspace_bytes': (_c.c_size_t, []),
    'stof_kuleshov_train_final_bwd': (_c.c_int, [_c.POINTER(KuleshovDesc)] + [_c.c_void_p] * 3 + [_c.c_int64] + [_c.c_void_p] * 4 +
                                      [_c.c_size_t, _c.c_void_p]),
    'stof_kuleshov_train_gather_up': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_uint64, _c.c_uint32,
                                                 _c.c_uint32, _c.c_int32, _c.c_double, _c.c_void_p, _c.c_void_p]),
    'stof_kuleshov_train_gather_down': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64,
                                                   _c.c_int32, _c.c_void_p, _c.c_void_p]),
    'stof_kuleshov_train_gather_bott': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_uint64, _c.c_uint32, _c.c_uint32,
                                                   _c.c_double, _c.c_void_p, _c.c_void_p]),
    'stof_kuleshov_train_bn_bwd': (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int64, _c.c_int32, _c.c_int32] + [_c.c_void_p] * 4 +
                                   [_c.c_size_t, _c.c_void_p]),
    'stof_kuleshov_train_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int64, _c.c_int64] + [_c.c_int32] * 3),
    'stof_kuleshov_train_wgrad': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int64] + [_c.c_int32] * 4 +
                                  [_c.c_void_p] * 3 + [_c.c_size_t, _c.c_void_p]),
    'stof_kuleshov_train_dgrad_workspace_bytes': (_c.c_size_t, [_c.c_int64, _c.c_int64] + [_c.c_int32] * 3),
    'stof_kuleshov_train_dgrad': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64] + [_c.c_int32] * 4 + [_c.c_void_p] * 2 + [_c.c_int64] +
                                  [_c.c_void_p] * 2 + [_c.c_size_t, _c.c_void_p]),
    'stof_kuleshov_train_down0_bwd_workspace_bytes': (_c.c_size_t, []),
    'stof_kuleshov_train_down0_bwd': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64] +
                                      [_c.c_void_p] * 3 + [_c.c_int64, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_iq2rf': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_double, _c.c_double, _c.c_double,
                              _c.c_int32, _c.c_void_p]),
    'stof_augment': (_c.c_int, [_c.POINTER(AugmentDesc), _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p,
                                _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_augment_uniforms': (_c.c_int, [_c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64,
                                         _c.c_void_p]),
    'stof_das_tx_distance': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                        _c.c_void_p]),
    'stof_das_beamform_host': (_c.c_int, [_c.POINTER(DasDesc), _c.c_void_p] + [_c.c_int64] * 4 + [_c.c_void_p] * 3 + [_c.c_int64] +
                               [_c.c_void_p] * 3),
    'stof_das_beamform': (_c.c_int, [_c.POINTER(DasDesc), _c.c_void_p] + [_c.c_int64] * 4 + [_c.c_void_p] * 3 + [_c.c_int64] +
                          [_c.c_void_p] * 4),
    'stof_das_workspace_bytes': (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    'stof_das_bmode': (_c.c_int, [_c.c_int32, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_toa_rmse': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_float,
                                 _c.c_void_p, _c.c_void_p]),
    'stof_train_repack_floats': (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32]),
    'stof_train_repack': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_conv': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int32]),
    'stof_train_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_float, _c.c_int32, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_conv1': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_conv1_wgrad_workspace_bytes': (_c.c_size_t, []),
    'stof_train_conv1_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_wgrad_batch_workspace_bytes': (_c.c_size_t, [_c.c_int32, _c.c_int32]),
    'stof_train_wgrad_batch': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_int64, _c.c_int32,
                                          _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_conv1_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float, _c.c_void_p]),
    'stof_train_conv1_c': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_void_p]),
    'stof_train_conv1_c_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32, _c.c_int32]),
    'stof_train_conv1_c_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int64, _c.c_int32,
                                            _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_conv1_c_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_float, _c.c_void_p]),
    'stof_train_edsr_in': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_edsr_in_wgrad_workspace_bytes': (_c.c_size_t, []),
    'stof_train_edsr_in_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64,
                                            _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_edsr_in_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float,
                                            _c.c_void_p]),
    'stof_train_edsr_out': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p]),
    'stof_train_edsr_out_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p]),
    'stof_train_edsr_out_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32]),
    'stof_train_edsr_out_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_float,
                                             _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_espcn_repack_floats': (_c.c_size_t, []),
    'stof_train_espcn_repack': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_train_espcn_in': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_espcn_mid': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_espcn_out': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p]),
    'stof_train_espcn_out_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32]),
    'stof_train_espcn_out_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32,
                                              _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_espcn_out_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32,
                                              _c.c_void_p]),
    'stof_train_espcn_in_wgrad_workspace_bytes': (_c.c_size_t, []),
    'stof_train_espcn_in_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float,
                                             _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_espcn_in_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float, _c.c_void_p]),
    'stof_train_upsample_bwd_c': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_sweep_blob_bytes': (_c.c_size_t, [_c.c_void_p]),
    'stof_train_sweep_pack': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_train_sweep_dump_floats': (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    'stof_train_sweep': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_sweep_bwd_pack': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_train_sweep_bwd': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_pool': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_conv_last_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p]),
    'stof_train_sgb_dgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32]),
    'stof_train_sgb_contract_dgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                                 _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_sgb_wgrad_workspace_bytes': (_c.c_size_t, [_c.c_int32]),
    'stof_train_sgb_contract_wgrad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                                 _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_pool_bwd': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_sgb_blob_bytes': (_c.c_size_t, []),
    'stof_train_sgb_contract_pool': (_c.c_int, [_c.c_void_p] * 8 + [_c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_upsample_add': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_upsample_add_c': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_upsample_bwd': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p]),
    'stof_train_loss': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float, _c.c_float, _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_train_loss_target': (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_train_loss_grad': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_float, _c.c_float, _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    'stof_train_add': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    'stof_train_add_split': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    'stof_train_to_split_rows': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    'stof_train_add_split2': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    'stof_train_conv_last_dgrad_split': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_void_p]),
    'stof_train_sweep_split': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_sweep_bwd_split': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p]),
    'stof_train_wgrad_batch_split': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_uint32, _c.c_uint32, _c.c_int64,
                                                _c.c_int64, _c.c_int32, _c.c_float, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    'stof_train_adamw': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_int64, _c.c_void_p]),
    'stof_train_adamw_guarded': (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib():
    """Load the shared library once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StofnetLibraryMissing(
                f'{LIB_PATH} not found: build the HIP extension first (python -m stofnet_amd.build). '
                'stofnet_amd has no CPU/PyTorch fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def status_string(code: int) -> str:
    return lib().stof_status_string(int(code)).decode()


def check(code: int, what: str = ''):
    """Convert a stof_status into the exception class the reference would raise."""
    if code == STOF_OK:
        return
    msg = f'{what}: {status_string(code)}' if what else status_string(code)
    if code in (STOF_ERR_ODD_SGB_REMAINDER, STOF_ERR_CHANNELS, STOF_ERR_HIP, STOF_ERR_WORKSPACE, STOF_ERR_POOL_EMPTY):
        raise RuntimeError(msg)          # torch raises RuntimeError for shape mismatches
    if code == STOF_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise ValueError(msg)


def call(name: str, *args):
    """Entry `name` of the library on plain Python arguments: a ctypes structure goes by reference, a tensor as its device
    pointer, None (a NULL pointer), numbers and ctypes arrays as they are.  An int result is a stof_status and is checked under
    `name`; any other result (a size) is returned."""
    fn = getattr(lib(), name)
    out = fn(*[ptr(a) if isinstance(a, torch.Tensor) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args])
    if _SIGNATURES[name][0] is not ctypes.c_int:
        return out
    check(out, name)


def require_device(t: torch.Tensor, name: str = 'tensor') -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch.Tensor')
    if t.device.type != 'cuda':
        raise RuntimeError(f'{name} is on {t.device}: stofnet_amd runs on a ROCm device only '
                           '(no CPU fallback; use oracle/ for a CPU check)')
    return t


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())
