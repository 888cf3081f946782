"""ctypes binding of libpatchioner_hip.so (the C ABI declared in include/patchioner_hip.h).

This is the stub a maintainer of the reference would add: plain pointers and
sizes, device pointers taken from torch tensors with ``.data_ptr()``, the stream from
``torch.cuda.current_stream().cuda_stream``.  There is NO fallback: if the library is missing or a call
fails, a ``PioError`` is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIO_LIB_PATH") or os.path.join(_HERE, "libpatchioner_hip.so")   # PIO_LIB_PATH: A/B builds of the same ABI (tools/microbench)


class PioError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libpatchioner_hip error %d: %s" % (code, msg))
        self.code = code


PIO_ERR_UNKNOWN_WEIGHT = -4


class PioConfig(ctypes.Structure):
    _fields_ = [
        ("embed_dim", c_int32), ("depth", c_int32), ("num_heads", c_int32), ("patch_size", c_int32),
        ("num_registers", c_int32), ("pretrain_grid", c_int32), ("crop_dim", c_int32), ("vit_ln_eps", c_float),
        ("readout_heads", c_int32), ("readout_scale", c_float),
        ("dec_layers", c_int32), ("dec_heads", c_int32), ("dec_embd", c_int32), ("dec_vocab", c_int32),
        ("dec_positions", c_int32), ("prefix_size", c_int32), ("dec_ln_eps", c_float),
        ("max_batch", c_int32), ("max_prefixes", c_int32), ("max_steps", c_int32),
        ("vit_operand_type", c_int32), ("device", c_int32),
        ("vit_arch", c_int32), ("vit_out_dim", c_int32),
        ("rn_layers", c_int32 * 4), ("rn_width", c_int32), ("rn_attnpool_spatial", c_int32),
        ("vit_self_only_layers", c_int32),
    ]


class PioTextConfig(ctypes.Structure):
    _fields_ = [
        ("device", c_int32), ("width", c_int32), ("layers", c_int32), ("heads", c_int32), ("context_length", c_int32),
        ("vocab_size", c_int32), ("embed_dim", c_int32), ("max_texts", c_int32), ("operand_type", c_int32),
    ]


class PioTestGemmArgs(ctypes.Structure):
    """pio_test_gemm_args (the test hooks' mirror of the GEMM launch arguments)."""
    _fields_ = [
        ("A", c_void_p), ("W", c_void_p), ("bias", c_void_p), ("M", c_int32), ("N", c_int32), ("K", c_int32), ("lda", c_int32),
        ("x", c_void_p), ("pos", c_void_p), ("out16", c_void_p), ("q", c_void_p), ("k", c_void_p), ("vT", c_void_p),
        ("qkv_last", c_void_p), ("T", c_int32), ("Tp", c_int32), ("Tk", c_int32), ("G", c_int32), ("n2", c_int32), ("D", c_int32),
        ("H", c_int32), ("act", c_int32), ("pf", c_void_p), ("pf_bytes", c_int32),
    ]


# every symbol include/patchioner_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "pio_last_error": (c_char_p, []),
    "pio_version": (c_char_p, []),
    "pio_stream_create": (c_int32, [c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "pio_stream_destroy": (c_int32, [c_void_p]),
    "pio_create": (c_int32, [POINTER(PioConfig), POINTER(c_void_p)]),
    "pio_destroy": (c_int32, [c_void_p]),
    "pio_clone_decoder": (c_int32, [c_void_p, POINTER(c_void_p)]),
    "pio_load_weight": (c_int32, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int32]),
    "pio_finalize_weights": (c_int32, [c_void_p]),
    "pio_set_memory_bank": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, POINTER(c_int64)]),
    "pio_set_memory_bank_device": (c_int32, [c_void_p, c_void_p, c_int64, c_int32]),
    "pio_vit_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "pio_vit_forward_rows": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pio_region_reduce_rows": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_void_p, c_void_p]),
    "pio_host_trace_quads": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "pio_vit_forward_regions": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "pio_region_masks": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p]),
    "pio_cls_attention": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "pio_trace_grids": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_bbox_weights": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p,
                                   c_void_p, c_int32, c_void_p, c_void_p]),
    "pio_region_reduce": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_float, c_void_p,
                                    c_void_p]),
    "pio_gaussian_map": (c_int32, [c_void_p, c_float, c_void_p, c_void_p]),
    "pio_mem_project": (c_int32, [c_void_p, c_void_p, c_int32, c_float, c_int32, c_void_p, c_int32, c_void_p,
                                  c_void_p]),
    "pio_viecap_prompt_length": (c_int32, [c_void_p]),
    "pio_viecap_set_entities": (c_int32, [c_void_p, c_void_p, c_int32, c_int32]),
    "pio_viecap_mapping": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "pio_viecap_entity_logits": (c_int32, [c_void_p, c_void_p, c_int32, c_float, c_void_p, c_void_p]),
    "pio_lm_score": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_viecap_decode": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_viecap_build_prompt": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_viecap_compose_prompts": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                             c_int32, c_int32, c_int32, c_float, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                             c_void_p, c_void_p]),
    "pio_viecap_decode_ragged": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                           c_void_p]),
    "pio_lm_prefill": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_lm_advance": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_beam_select": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "pio_viecap_build_prompt_ragged": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                 c_void_p]),
    "pio_lm_beam_search": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "pio_clipcap_mapping": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_clipcap_prefix_length": (c_int32, [c_void_p]),
    "pio_nucleus_sample": (c_int32, [c_void_p, c_void_p, c_int32, c_float, c_float, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pio_lm_sample": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_uint64, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "pio_mem_topk": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "pio_text_project": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                   c_void_p, c_void_p, c_void_p]),
    "pio_revert_transformation": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "pio_decode_greedy": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "pio_decode_greedy_stop": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, POINTER(c_int32), c_void_p]),
    "pio_viecap_decode_stop": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                         POINTER(c_int32), c_void_p]),
    "pio_profile_enable": (c_int32, [c_void_p, c_int32]),
    "pio_profile_read": (c_int32, [c_void_p, c_int32, POINTER(c_double), POINTER(c_int64), POINTER(c_double),
                                   POINTER(c_double)]),
    "pio_bbox_double_dino": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_ctx_clean": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, c_void_p,
                                c_void_p]),
    "pio_preprocess": (c_int32, [c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int32), c_int32, c_int32, c_int32, c_int32,
                                 c_void_p, c_void_p]),
    "pio_text_create": (c_int32, [POINTER(PioTextConfig), POINTER(c_void_p)]),
    "pio_text_destroy": (c_int32, [c_void_p]),
    "pio_text_load_weight": (c_int32, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int32]),
    "pio_text_finalize": (c_int32, [c_void_p]),
    "pio_text_encode": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_num_tokens": (c_int32, [c_void_p]),
    "pio_grid_side": (c_int32, [c_void_p]),
    "pio_bank_rows": (c_int64, [c_void_p]),
    "pio_bank_form": (c_int32, [c_void_p]),
    "pio_host_interpolate_pos_embed": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "pio_host_interpolate_pos_embed_plain": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_double, c_void_p]),
    "pio_host_pil_ksize": (c_int32, [c_int32, c_int32]),
    "pio_host_pil_table": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_host_philox4x32": (c_int32, [POINTER(c_uint32), c_uint32, c_uint32, POINTER(c_uint32)]),
    "pio_host_philox_uniform": (c_int32, [c_uint64, c_uint32, c_uint32, POINTER(c_float)]),
    "pio_host_philox_uniforms": (c_int32, [c_uint64, c_uint32, c_int32, c_int32, c_void_p]),
    "pio_host_ln_fold": (c_int32, [c_void_p, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pio_test_vit_gemm": (c_int32, [c_int32, c_int32, c_int32, POINTER(PioTestGemmArgs), POINTER(c_int32), c_void_p]),
    "pio_test_gemm_route": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "pio_test_vit_vonly": (c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, POINTER(c_int32), c_void_p]),
    "pio_test_attention": (c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                     c_int32, c_int32, c_float, c_void_p, c_void_p]),
    "pio_test_layernorm": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                     c_int32, c_void_p]),
    "pio_test_im2col_alpha": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_conv": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "pio_test_avgpool": (c_int32, [c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_attnpool_in": (c_int32, [c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_nucleus_sample": (c_int32, [c_void_p, c_int32, c_int32, c_float, c_float, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "pio_test_dec_workspace": (c_int32, [POINTER(c_int64), POINTER(c_int32)]),
    "pio_test_dec_split_weights": (c_int32, [c_void_p, c_int64, c_void_p, POINTER(c_float), c_void_p]),
    "pio_test_dec_gemm": (c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                    c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pio_test_dec_attention": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "pio_test_beam_select": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "pio_test_beam_step": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_lm_head_rows": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                        c_void_p, c_void_p]),
    "pio_test_project_pass": (c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32,
                                        c_float, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "pio_test_bank_prep": (c_int32, [c_void_p, c_int64, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pio_test_dec_stop_scan": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "pio_test_dec_stop_pad": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_sgemm": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_float, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                 c_int32, c_int32, c_void_p]),
    "pio_test_attention_f32": (c_int32, [c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p,
                                         c_void_p]),
    "pio_test_layernorm_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_pointwise_f32": (c_int32, [c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "pio_test_im2col_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_embed_scatter_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "pio_test_text_embed": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "pio_test_text_pool": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float,
                                     c_void_p, c_void_p, c_void_p]),
}

_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Loads the library (once).  ``import torch`` first so both share torch's bundled HIP runtime."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PioError(-100, "%s not found: run `python patchioner_amd/build.py` (hipcc, gfx950); "
                             "there is no CPU fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  (loads libamdhip64 with the soname our library asks for)
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise PioError(rc, load().pio_last_error().decode("utf-8", "replace"))


def ptr(t) -> Optional[int]:
    """Device/host pointer of a contiguous torch tensor (None stays NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor crossing the C ABI must be contiguous"
    return t.data_ptr()
