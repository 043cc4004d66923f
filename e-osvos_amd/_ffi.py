"""ctypes binding of libeosvos.so (include/eosvos.h).

`cffi` is not installed in the target image, so the thin shim is `ctypes` (stdlib).
There is deliberately no fallback: if the library is missing or a call fails, an
exception is raised -- a silent CPU/eager path would void every parity claim.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EOSVOS_LIB') or os.path.join(_HERE, 'libeosvos.so')   # EOSVOS_LIB: A/B-test builds

c_float_p = ctypes.c_void_p  # device pointers travel as integers (tensor.data_ptr())
_E = ctypes.c_void_p


class View(ctypes.Structure):
    """include/eosvos.h eosvos_view: a pixel-major view (first element, floats per pixel) and the tensor it is a slice of."""
    _fields_ = [('p', ctypes.c_void_p), ('ld', ctypes.c_int), ('key', ctypes.c_void_p), ('ldkey', ctypes.c_int)]


class ConvViews(ctypes.Structure):
    """include/eosvos.h eosvos_conv_views."""
    _fields_ = ([(n, ctypes.c_int) for n in ('algo', 'B', 'H', 'W', 'Cin', 'Cout', 'k', 'stride', 'dil', 'pad')] +
                [('w_oihw', ctypes.c_void_p), ('scale', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('passes', ctypes.c_int),
                 ('x', View), ('y', View), ('res', View), ('relu', ctypes.c_int), ('y_m8', ctypes.c_void_p),
                 ('g', View), ('gx', View), ('add', View), ('accum', ctypes.c_int), ('mask_c0', ctypes.c_int),
                 ('gx_m8', ctypes.c_void_p), ('dw_oihw', ctypes.c_void_p),
                 ('slot_bits', ctypes.c_uint * 2), ('slot_valid', ctypes.c_int * 2),
                 ('src_slot_bits', ctypes.c_uint * 2), ('src_slot_valid', ctypes.c_int * 2), ('fwd_slices', ctypes.c_int)])


VIEWS_FWD, VIEWS_DGRAD, VIEWS_WGRAD = 1, 2, 4

_SIGNATURES = {
    # name: (restype, argtypes)
    'eosvos_version': (ctypes.c_char_p, []),
    'eosvos_last_error': (ctypes.c_char_p, []),
    'eosvos_set_matrix_mode': (ctypes.c_int, [ctypes.c_int]),
    'eosvos_get_matrix_mode': (ctypes.c_int, []),
    'eosvos_set_presplit': (ctypes.c_int, [ctypes.c_int]),
    'eosvos_plan_fingerprint': (ctypes.c_int, [_E, ctypes.POINTER(ctypes.c_uint64)]),
    'eosvos_set_engine_matrix_mode': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_get_engine_matrix_mode': (ctypes.c_int, [_E]),
    'eosvos_set_wg_budget': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_set_side_stream': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_num_convs': (ctypes.c_int, [ctypes.c_int]),
    'eosvos_conv_info': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_param_count': (ctypes.c_int64, [ctypes.c_int]),
    'eosvos_lr_count': (ctypes.c_int64, [ctypes.c_int]),
    'eosvos_norm_count': (ctypes.c_int64, [ctypes.c_int]),
    'eosvos_create': (ctypes.c_int, [ctypes.POINTER(_E), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'eosvos_create_ex': (ctypes.c_int, [ctypes.POINTER(_E), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    'eosvos_destroy': (ctypes.c_int, [_E]),
    'eosvos_synchronize': (ctypes.c_int, [_E]),
    'eosvos_debug_check_guards': (ctypes.c_int, [_E]),
    'eosvos_set_init': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_set_lr': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_lr_store_count': (ctypes.c_int64, [ctypes.c_int, ctypes.c_int]),
    'eosvos_set_lr_state': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_int, c_float_p]),
    'eosvos_set_loss': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_last_loss': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_loss_tensors': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, c_float_p, ctypes.c_int64, c_float_p]),
    'eosvos_loss_ignore': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, ctypes.c_int, ctypes.c_float, c_float_p]),
    'eosvos_loss_tensors_ignore': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, c_float_p, ctypes.c_int64, ctypes.c_float,
                                                  c_float_p]),
    'eosvos_set_loss_ignore': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_float]),
    'eosvos_set_loss_sum': (ctypes.c_int, [_E, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)]),
    'eosvos_loss_sum': (ctypes.c_int, [_E, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float), c_float_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_float, c_float_p]),
    'eosvos_loss_sum_tensors': (ctypes.c_int, [_E, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float),
                                               c_float_p, c_float_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, c_float_p,
                                               c_float_p]),
    'eosvos_last_loss_terms': (ctypes.c_int, [_E, c_float_p, ctypes.POINTER(ctypes.c_int)]),
    'eosvos_set_loss_bootstrap': (ctypes.c_int, [_E, ctypes.c_float]),
    'eosvos_set_loss_boundary': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_boundary_f': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_float, c_float_p, c_float_p]),
    'eosvos_set_loss_surface': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_surface_loss': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_float), c_float_p, c_float_p]),
    'eosvos_surface_weights': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, c_float_p]),
    'eosvos_set_loss_potts': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float]),
    'eosvos_potts_loss': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_float, ctypes.c_float, c_float_p, c_float_p]),
    'eosvos_set_loss_cldice': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_cldice_loss': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_float), c_float_p, c_float_p]),
    'eosvos_soft_skeleton': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_float), c_float_p]),
    'eosvos_propagation_targets': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
                                                  ctypes.c_float, c_float_p, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_warp_affine': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_int, c_float_p, ctypes.POINTER(ctypes.c_int)]),
    'eosvos_warp_affine_hw': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_int, c_float_p, ctypes.POINTER(ctypes.c_int)]),
    'eosvos_davis_counts': (ctypes.c_int, [_E, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_crf_labels': (ctypes.c_int, [_E, c_float_p, c_float_p] + [ctypes.c_int] * 7 + [ctypes.c_float] * 5 +
                          [ctypes.c_void_p, c_float_p]),
    'eosvos_label_components': (ctypes.c_int, [_E, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    'eosvos_filter_components': (ctypes.c_int, [_E, ctypes.c_void_p] + [ctypes.c_int] * 8 +
                                 [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_fill_holes': (ctypes.c_int, [_E, ctypes.c_void_p] + [ctypes.c_int] * 7 +
                          [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_superpixels': (ctypes.c_int, [_E, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]),
    'eosvos_snap_labels': (ctypes.c_int, [_E, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 +
                           [ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_block_motion': (ctypes.c_int, [_E, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]),
    'eosvos_warp_labels': (ctypes.c_int, [_E, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    'eosvos_zoom_boxes': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float] +
                          [ctypes.c_int] * 5 + [ctypes.c_void_p]),
    'eosvos_zoom_crop': (ctypes.c_int, [_E, c_float_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [c_float_p]),
    'eosvos_zoom_accumulate': (ctypes.c_int, [_E, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                              c_float_p]),
    'eosvos_zoom_blend': (ctypes.c_int, [_E, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                         c_float_p, c_float_p]),
    'eosvos_lucid_plate': (ctypes.c_int, [_E, c_float_p, c_float_p] + [ctypes.c_int] * 4 + [c_float_p]),
    'eosvos_lucid_compose': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p] + [ctypes.c_int] * 4 +
                             [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), c_float_p, c_float_p,
                              ctypes.POINTER(ctypes.c_int32)]),
    'eosvos_lucid_compose_layers': (ctypes.c_int, [_E, c_float_p, ctypes.c_void_p, c_float_p] + [ctypes.c_int] * 4 +
                                    [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                     ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double), ctypes.c_int, c_float_p,
                                     c_float_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    'eosvos_distance_sq': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_void_p]),
    'eosvos_adapt_targets': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] +
                             [ctypes.c_float] * 3 + [ctypes.c_int] * 2 + [ctypes.c_float, c_float_p, ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_set_norm': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_float]),
    'eosvos_reset': (ctypes.c_int, [_E]),
    'eosvos_get_params': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_set_params': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_snapshot_params': (ctypes.c_int, [_E]),
    'eosvos_restore_params': (ctypes.c_int, [_E]),
    'eosvos_forward': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, c_float_p]),
    'eosvos_loss_bce': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, c_float_p]),
    'eosvos_loss': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, ctypes.c_int, c_float_p]),
    'eosvos_bce': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int64, c_float_p, c_float_p]),
    'eosvos_backward_step': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_finetune_step': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_float)]),
    'eosvos_keep_grads': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_get_grads': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_debug_gsum': (ctypes.c_int, [_E, c_float_p]),
    'eosvos_infer': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, c_float_p]),
    'eosvos_infer_view': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int]),
    'eosvos_tta_accumulate': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                             c_float_p, ctypes.c_int, ctypes.c_int]),
    'eosvos_resize_frames': (ctypes.c_int, [_E, c_float_p] + [ctypes.c_int] * 6 + [c_float_p]),
    'eosvos_merge_labels': (ctypes.c_int, [_E, c_float_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]),
    'eosvos_meta_task_begin': (ctypes.c_int, [_E]),
    'eosvos_meta_grad': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, c_float_p,
                                        ctypes.POINTER(ctypes.c_float)]),
    'eosvos_meta_grad_ex': (ctypes.c_int, [_E, c_float_p, c_float_p, ctypes.c_int, c_float_p,
                                           ctypes.POINTER(ctypes.c_float), ctypes.c_float, ctypes.c_int]),
    'eosvos_radam_step': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_int64,
                                         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float]),
    'eosvos_clamp': (ctypes.c_int, [_E, c_float_p, ctypes.c_int64, ctypes.c_float, ctypes.c_float]),
    'eosvos_outer_step': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_int, ctypes.c_int64, ctypes.c_int64]),
    'eosvos_alias_state': (ctypes.c_int, [_E, _E]),
    'eosvos_unalias_state': (ctypes.c_int, [_E]),
    'eosvos_set_trainable_from': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_comm_unique_id': (ctypes.c_int, [ctypes.c_void_p]),
    'eosvos_comm_init_rank': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    'eosvos_comm_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'eosvos_allreduce_sum': (ctypes.c_int, [_E, c_float_p, ctypes.c_int64, ctypes.c_void_p]),
    'eosvos_time_hot_kernel': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                              ctypes.POINTER(ctypes.c_double)]),
    'eosvos_bench_conv': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]),
    'eosvos_mfma_probe': (ctypes.c_int, [_E, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                         ctypes.POINTER(ctypes.c_double)]),
    'eosvos_profile_launches': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_profile_read': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64),
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int)]),
    'eosvos_test_conv_plan_log': (ctypes.c_int, [_E, ctypes.c_int]),
    'eosvos_test_conv_plan_log_read': (ctypes.c_int, [_E, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                                      ctypes.POINTER(ctypes.c_int)]),
    'eosvos_debug_tensor': (ctypes.c_int, [_E, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.POINTER(ctypes.c_int64)]),
    'eosvos_test_conv': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                        ctypes.c_int] + [ctypes.c_int] * 9 + [c_float_p]),
    'eosvos_test_conv_bwd': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p] + [ctypes.c_int] * 9 +
                             [c_float_p, c_float_p]),
    'eosvos_test_conv_algo': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                             ctypes.c_int] + [ctypes.c_int] * 9 + [c_float_p]),
    'eosvos_test_conv_bwd_algo': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_void_p] +
                                  [ctypes.c_int] * 9 + [c_float_p, c_float_p]),
    'eosvos_test_conv_views': (ctypes.c_int, [_E, ctypes.POINTER(ConvViews)]),
    'eosvos_test_aspp_dgrad': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, ctypes.c_void_p, c_float_p, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint),
                                              ctypes.POINTER(ctypes.c_int)]),
    'eosvos_test_groupnorm': (ctypes.c_int, [_E, ctypes.c_int, c_float_p, ctypes.c_int, c_float_p, ctypes.c_int, c_float_p,
                                             c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_float, c_float_p, ctypes.c_int, c_float_p, ctypes.c_void_p,
                                             ctypes.c_int]),
    'eosvos_test_maxpool': (ctypes.c_int, [_E, c_float_p] + [ctypes.c_int] * 4 + [c_float_p, ctypes.c_void_p, c_float_p, c_float_p]),
    'eosvos_test_resize': (ctypes.c_int, [_E] + [ctypes.c_int] * 7 + [c_float_p, ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int]),
    'eosvos_test_aspp_pool': (ctypes.c_int, [_E] + [ctypes.c_int] * 4 + [c_float_p] * 4 + [ctypes.c_int] + [c_float_p] * 3 +
                              [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, c_float_p, ctypes.c_int] + [c_float_p] * 4 +
                              [ctypes.c_int]),
    'eosvos_test_head': (ctypes.c_int, [_E, c_float_p, c_float_p, c_float_p, ctypes.c_int64, ctypes.c_int] + [c_float_p] * 4),
    'eosvos_test_wgrad_presplit': (ctypes.c_int, [c_float_p] * 8 + [ctypes.c_int] * 15 + [ctypes.c_void_p]),
}

_lib = None


class EosvosError(RuntimeError):
    pass


def load():
    """Load libeosvos.so (once) and declare every prototype of include/eosvos.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EosvosError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_SIGNATURES)


def check(rc):
    if rc != 0:
        raise EosvosError(load().eosvos_last_error().decode() or f'eosvos call failed ({rc})')
