"""ctypes binding of libsbk_hip.so (include/sbk.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the HIP stream; every
numeric op on the hot path is one of the C-ABI entry points below.  There is NO
CPU fallback: a CPU tensor, or a missing library, raises.
"""

from __future__ import annotations

import collections
import contextlib
import ctypes
import math
import os
import threading
import weakref
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsbk_hip.so")

ACT_NONE, ACT_SWISH, ACT_GELU, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2, 3, 4

_lib = None


class SbkError(RuntimeError):
    pass


class DecoderLayer(ctypes.Structure):  # sbk_decoder_layer
    _fields_ = [(n, c_void_p) for n in (
        "ln1_g", "ln1_b", "sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ln2_g", "ln2_b", "ca_in_w", "ca_in_b",
        "ca_out_w", "ca_out_b", "ln3_g", "ln3_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b", "sa_in_wf", "sa_in_bf", "ca_q_wf",
        "ca_q_bf", "ff1_wf", "ff1_bf", "ca_kv_w3", "sa_in_wp", "sa_out_wp", "ca_q_wp", "ca_out_wp", "ff1_wp", "ff2_wp",
        "sa_in_wfp", "ca_q_wfp", "ff1_wfp")]


class DecoderWeights(ctypes.Structure):  # sbk_decoder_weights
    _fields_ = [("layers", POINTER(DecoderLayer)), ("emb", c_void_p), ("pe", c_void_p), ("final_ln_g", c_void_p),
                ("final_ln_b", c_void_p), ("seq_w", c_void_p), ("seq_b", c_void_p), ("seq_wf", c_void_p),
                ("seq_bf", c_void_p), ("d_model", c_int32),
                ("nhead", c_int32), ("d_ffn", c_int32), ("n_layers", c_int32), ("vocab", c_int32),
                ("max_len", c_int32), ("ffn_act", c_int32), ("ln_eps", c_float), ("emb_scale", c_float),
                ("seq_w3", c_void_p), ("seq_wp", c_void_p), ("seq_wfp", c_void_p)]


class LMLayer(ctypes.Structure):  # sbk_lm_layer
    _fields_ = [(n, c_void_p) for n in ("in_w", "in_b", "out_w", "out_b", "ln1_g", "ln1_b", "ff1_w", "ff1_b", "ff2_w",
                                        "ff2_b", "ln2_g", "ln2_b")]


class LMWeights(ctypes.Structure):  # sbk_lm_weights
    _fields_ = [("layers", POINTER(LMLayer))] + [(n, c_void_p) for n in (
        "emb", "pe", "final_ln_g", "final_ln_b", "out0_w", "out0_b", "out_ln_g", "out_ln_b", "out2_w", "out2_b")] + [
        (n, c_int32) for n in ("d_model", "nhead", "d_ffn", "n_layers", "vocab", "max_len", "ffn_act",
                               "normalize_before", "pad_idx")] + [("ln_eps", c_float)]


class SearchConfig(ctypes.Structure):  # sbk_search_config
    _fields_ = [("bos", c_int32), ("eos", c_int32), ("blank", c_int32), ("beam", c_int32), ("min_steps", c_int32),
                ("max_steps", c_int32), ("length_normalization", c_int32), ("using_eos_threshold", c_int32),
                ("check_every", c_int32), ("overlap_ctc", c_int32), ("ctc_weight", c_float), ("temperature", c_float),
                ("eos_threshold", c_float), ("minus_inf", c_float), ("lm_weight", c_float), ("lm_temperature", c_float),
                ("lm", POINTER(LMWeights)), ("topk", c_int32), ("utt_min_steps", c_void_p),
                ("utt_max_steps", c_void_p), ("graph_mode", c_int32), ("ctc_candidates", c_int32),
                ("ctc_window_size", c_int32), ("prompt", c_void_p), ("prompt_len", c_int32), ("temperature_post", c_int32), ("logit_bias", c_void_p),
                ("first_bias", c_void_p), ("probe_pos", c_int32), ("probe_token", c_int32), ("out_probe", c_void_p),
                ("ctc_w3", c_void_p)]


class CTCBeamConfig(ctypes.Structure):  # sbk_ctc_beam_config
    _fields_ = [("blank", c_int32), ("beam_size", c_int32), ("topk", c_int32), ("prune_history", c_int32),
                ("beam_prune_logp", c_float), ("token_prune_min_logp", c_float), ("log_blank_skip_threshold", c_float),
                ("char_base1", ctypes.c_uint32), ("char_base2", ctypes.c_uint32), ("space_code", ctypes.c_uint32)]


class CTCLMTables(ctypes.Structure):  # sbk_ctc_lm_tables
    _fields_ = [("strings", c_void_p), ("unigrams", c_void_p), ("ngrams", c_void_p), ("n_string_slots", c_int32),
                ("n_words", c_int32), ("n_ngram_slots", c_int32), ("order", c_int32), ("unk_id", c_int32),
                ("bos_id", c_int32), ("score_boundary", c_int32), ("alpha", ctypes.c_double), ("beta", ctypes.c_double),
                ("unk_score_offset", ctypes.c_double), ("log10_e", ctypes.c_double)]


TRANSDUCER_MAX_LAYERS = 4
ACT_TANH = 5  # SBK_ACT_TANH (the transducer joint only)


class TransducerWeights(ctypes.Structure):  # sbk_transducer_weights
    _fields_ = [("emb_ih", c_void_p)] + [(n, c_void_p * TRANSDUCER_MAX_LAYERS) for n in ("w_ih", "w_hh", "b_ih", "b_hh")] + [
        (n, c_void_p) for n in ("proj", "proj_b", "out", "out_b")] + [
        (n, c_int32) for n in ("n_layers", "hidden", "joint", "vocab", "n_emb")]


class TransducerConfig(ctypes.Structure):  # sbk_transducer_config
    _fields_ = [(n, c_int32) for n in ("blank", "max_symbols_per_step", "start_from_blank", "frame_block", "act")]


TRANSDUCER_MAX_BEAM = 32  # SBK_TRANSDUCER_MAX_BEAM
TBEAM_CAPPED, TBEAM_TRUNCATED, TBEAM_EXHAUSTED = 1, 2, 4  # SBK_TBEAM_*: the bits of the beam search's status word


class TransducerBeamConfig(ctypes.Structure):  # sbk_transducer_beam_config
    _fields_ = [("blank", c_int32), ("beam_size", c_int32), ("nbest", c_int32), ("state_beam", c_float),
                ("expand_beam", c_float), ("max_expansions", c_int32), ("max_tokens", c_int32), ("act", c_int32)]


RNNLM_MAX_DNN = 2  # SBK_RNNLM_MAX_DNN


class RNNLMWeights(ctypes.Structure):  # sbk_rnnlm_weights
    _fields_ = [("emb_ih", c_void_p)] + [(n, c_void_p * TRANSDUCER_MAX_LAYERS) for n in ("w_ih", "w_hh", "b_ih", "b_hh")] + [
        (n, c_void_p * RNNLM_MAX_DNN) for n in ("dnn_w", "dnn_b", "ln_g", "ln_b")] + [("ln_eps", c_float * RNNLM_MAX_DNN)] + [
        (n, c_void_p) for n in ("out", "out_b")] + [
        (n, c_int32) for n in ("n_layers", "hidden", "n_dnn", "dnn", "vocab", "n_emb", "act")]


ATTN_RNN_MAX_LAYERS = 4  # SBK_ATTN_RNN_MAX_LAYERS


class AttnRNNWeights(ctypes.Structure):  # sbk_attn_rnn_weights
    _fields_ = [("emb", c_void_p)] + [(n, c_void_p * ATTN_RNN_MAX_LAYERS) for n in ("w_ih", "w_hh", "b_ih", "b_hh")] + [
        (n, c_void_p) for n in ("enc_w", "enc_b", "dec_w", "dec_b", "attn_v", "conv_w", "loc_w", "loc_b", "out_w", "out_b",
                                "proj_w", "proj_b", "fc_w", "fc_b")] + [
        (n, c_int32) for n in ("n_layers", "hidden", "in_dim", "attn_dim", "enc_dim", "channels", "kernel", "vocab", "n_emb")] + [
        ("scaling", c_float)]


def _declare(lib):
    p, i, f = c_void_p, c_int, c_float
    sig = {
        "sbk_attn_rnn_attend_workspace_bytes": ([i, i], ctypes.c_size_t),
        "sbk_attn_rnn_attend_f32": ([p] * 10 + [f, p, p, p, ctypes.c_size_t] + [i] * 7 + [p], c_int),
        "sbk_attn_rnn_attn_init_f32": ([p, p, p, i, i, i, p], c_int),
        "sbk_gru_cell_f32": ([p] * 6 + [i, i, p], c_int),
        "sbk_attn_rnn_greedy_workspace_bytes": ([POINTER(AttnRNNWeights), i, i], ctypes.c_size_t),
        "sbk_attn_rnn_greedy_f32": ([POINTER(AttnRNNWeights), p, p, p, ctypes.c_size_t, p, p, POINTER(c_int32)] + [i] * 6 + [p],
                                    c_int),
        "sbk_attn_rnn_decode_workspace_bytes": ([POINTER(AttnRNNWeights), i, i], ctypes.c_size_t),
        "sbk_attn_rnn_decode_f32": ([POINTER(AttnRNNWeights), p, p, p, p, ctypes.c_size_t, p, p, p, p, i, i, i, p], c_int),
        "sbk_abi_version": ([], c_int),
        "sbk_last_error": ([], c_char_p),
        "sbk_stream_workspace_bytes": ([], ctypes.c_size_t),
        "sbk_stream_workspace_set": ([p, p, ctypes.c_size_t], c_int),
        "sbk_stream_workspace_release": ([p], c_int),
        "sbk_prof_enable": ([i], None),
        "sbk_prof_reset": ([], None),
        "sbk_prof_report": ([ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t),
        "sbk_prof_ctc_psi_repeat_f32": ([p, p, p, p, p, i, i, i, i, i, i, POINTER(c_float), p], c_int),
        "sbk_prof_set_knob": ([i, i], None),
        "sbk_prof_get_knob": ([i], c_int),
        "sbk_ctc_scorer_workspace_bytes": ([i, i, i, i], ctypes.c_size_t),
        "sbk_ctc_scorer_reset_f32": ([p, p, p, ctypes.c_size_t, i, i, i, i, i, p], c_int),
        "sbk_ctc_scorer_score_f32": ([p, p, p, ctypes.c_size_t, p, i, p, i, p, i, i, i, i, i, i, p], c_int),
        "sbk_ctc_scorer_permute_f32": ([p, p, ctypes.c_size_t, p, p, p, i, p, i, i, i, i, i, i, p], c_int),
        "sbk_prof_persist_stamps": ([p, i], c_int),
        "sbk_prof_mfma_peak_f32": ([p, i, i, i, POINTER(c_float), p], c_int),
        "sbk_prof_stream_f32": ([p, p, ctypes.c_long, i, i, POINTER(c_float), p], c_int),
        "sbk_prof_gemm_repeat_f32": ([p, p, p, i, i, i, p, ctypes.c_size_t, i, POINTER(c_float), p], c_int),
        "sbk_pcm16_to_f32": ([p, p, ctypes.c_long, i, p], c_int),
        "sbk_fbank_f32": ([p, p, p, POINTER(c_int32), i, p, p, p, p, p, i, i, i, i, i, i, f, f, p, p, f, p], c_int),
        "sbk_whisper_log_mel_f32": ([p, p, p, POINTER(c_int32), i, p, p, p, p, p, p, i, i, i, i, i, i, p], c_int),
        "sbk_stft_f32": ([p, p, p, POINTER(c_int32), i, p, i, i, i, i, p], c_int),
        "sbk_spectral_magnitude_f32": ([p, p, ctypes.c_long, f, i, f, p], c_int),
        "sbk_amplitude_to_db_f32": ([p, p, i, ctypes.c_long, f, f, f, f, p], c_int),
        "sbk_input_norm_global_f32": ([p, p, p, p, i, i, f, p], c_int),
        "sbk_input_norm_stats_workspace_bytes": ([i, i], ctypes.c_size_t),
        "sbk_input_norm_stats_f32": ([p, p, p, p, i, i, i, i, i, f, i, p], c_int),
        "sbk_gemm_nt_f32": ([p, i, p, i, p, p, i, p, i, i, i, i, i, f, p, i, p], c_int),
        "sbk_f32_to_bf16": ([p, p, ctypes.c_long, p], c_int),
        "sbk_split_bf16x3": ([p, i, p, i, i, p], c_int),
        "sbk_gemm_nt_f32x3": ([p, i, p, p, p, i, p, i, i, i, i, i, f, p, i, p], c_int),
        "sbk_x3p_panel_bytes": ([i, i], ctypes.c_size_t),
        "sbk_split_x3p": ([p, i, p, i, i, p], c_int),
        "sbk_layernorm_x3p": ([p, p, p, p, i, i, f, i, p], c_int),
        "sbk_gemm_nt_x3r": ([p, i, p, p, p, i, p, i, i, i, i, i, f, p], c_int),
        "sbk_gemm_ln_nt_x3r": ([p, i, p, p, p, i, p, i, i, i, i, f, i, f, p], c_int),
        "sbk_quant_rows_fp8": ([p, i, p, p, i, i, p], c_int),
        "sbk_quant_rows_bf16_fp8": ([p, i, p, p, i, i, p], c_int),
        "sbk_layernorm_fp8o": ([p, p, p, p, p, i, i, f, i, p], c_int),
        "sbk_gemm_nt_fp8a": ([p, i, p, p, i, p, p, p, i, p, i, p, i, p, i, f, i, i, i, i, f, p], c_int),
        "sbk_input_norm_global_masked_f32": ([p, p, p, p, p, i, i, i, f, p], c_int),
        "sbk_gemm_nt_x3p": ([p, p, p, p, i, p, i, p, i, i, i, i, f, p, i, p], c_int),
        "sbk_gemm_nt_bf16": ([p, i, p, i, p, p, i, p, i, i, i, i, i, f, p, i, p], c_int),
        "sbk_gemm_nt_f16": ([p, i, p, i, p, p, i, p, i, i, i, i, i, f, p, i, p], c_int),
        "sbk_gemm_nt_bf16a": ([p, i, p, i, p, p, i, p, i, p, i, i, i, i, i, f, p], c_int),
        "sbk_layernorm_bf16o": ([p, p, p, p, i, i, f, i, p], c_int),
        "sbk_rope_attention_bf16o": ([p, p, p, p, p, i, i, i, i, i, f, i, i, p], c_int),
        "sbk_attention_bf16io_workspace_bytes": ([i, i, i], ctypes.c_size_t),
        "sbk_attention_bf16io": ([p, p, p, p, i, i, i, i, f, p], c_int),
        "sbk_f32_to_f16": ([p, p, ctypes.c_long, p], c_int),
        "sbk_gemm_nt_fp8": ([p, i, p, p, i, f, p, p, i, p, i, i, i, i, i, f, p, i, p], c_int),
        "sbk_f32_to_fp8": ([p, p, ctypes.c_long, f, p], c_int),
        "sbk_absmax_f32": ([p, ctypes.c_long, p, p], c_int),
        "sbk_gemm_ln_nt_f32": ([p, i, p, i, p, p, i, p, i, i, i, i, f, i, f, p], c_int),
        "sbk_gemm_nt_splitk_f32": ([p, i, p, i, p, p, i, p, i, i, i, i, i, f, p, ctypes.c_size_t, p], c_int),
        "sbk_conv_block_f32": ([p, p, p, p, p, p, i, i, i, i, i, f, f, p], c_int),
        "sbk_conv_block_k_layout": ([i, i, i], c_int),
        "sbk_conv_block_k_f32": ([p, p, p, p, p, p, i, i, i, i, i, i, i, f, f, p], c_int),
        "sbk_conv_block_res1x1_f32": ([p, p, p, p, p, f, p, p, p, p, f, p, i, i, i, i, i, f, p], c_int),
        "sbk_relpos_attention_f32": ([p, p, p, p, p, p, p, i, i, i, i, f, i, i, p], c_int),
        "sbk_rope_attention_f32": ([p, p, p, p, p, p, i, i, i, i, i, f, i, i, p], c_int),
        "sbk_rope_attention_bf16": ([p, p, p, p, p, i, i, i, i, i, f, i, i, p], c_int),
        "sbk_glu_dwconv_f32": ([p, p, p, p, i, i, i, i, i, p], c_int),
        "sbk_csgu_f32": ([p, p, p, f, p, p, p, p, i, i, i, i, i, p], c_int),
        "sbk_w2v_conv0_stats_workspace_bytes": ([i, i, i, i], ctypes.c_size_t),
        "sbk_w2v_conv0_stats_f32": ([p, p, p, i, f, f, p, p, p, ctypes.c_size_t, i, i, i, i, i, p], c_int),
        "sbk_w2v_conv0_f32": ([p, p, p, p, i, p, p, p, f, p, i, i, i, i, i, p], c_int),
        "sbk_w2v_posconv_f32": ([p, p, p, p, p, p, f, p, i, i, i, i, i, p], c_int),
        "sbk_w2v_utt_norm_f32": ([p, p, i, ctypes.c_long, f, p], c_int),
        "sbk_wavlm_attention_max_frames": ([], c_int),
        "sbk_wavlm_attention_f32": ([p, p, p, p, p, p, p, p, i, i, i, i, f, p], c_int),
        "sbk_hypermix_split_frames": ([], c_int),
        "sbk_hypermix_workspace_bytes": ([i, i, i, i], ctypes.c_size_t),
        "sbk_hypermix_f32": ([p] * 13 + [f, p, p, p, ctypes.c_size_t, i, i, i, i, i, p], c_int),
        "sbk_rnn_layer_route": ([i, i, i, i], c_int),
        "sbk_rnn_layer_f32": ([p] * 9 + [i] * 6 + [p], c_int),
        "sbk_crdnn_conv1_f32": ([p] * 6 + [i, i, i, i, f, f, p], c_int),
        "sbk_crdnn_im2col_f32": ([p, p, i, i, i, i, i, i, p], c_int),
        "sbk_crdnn_norm_pool_f32": ([p] * 4 + [i] * 6 + [f, f, p], c_int),
        "sbk_layernorm_f32": ([p, p, p, p, i, i, f, i, p], c_int),
        "sbk_log_softmax_f32": ([p, p, i, i, f, f, p], c_int),
        "sbk_ctc_greedy_decode_f32": ([p, p, p, p, i, i, i, i, p], c_int),
        "sbk_ctc_beam_search_workspace_bytes": ([i, i, i, i, i], ctypes.c_size_t),
        "sbk_ctc_beam_search_f32": ([p, p, p, i, POINTER(CTCBeamConfig), p, ctypes.c_size_t, p, p, p, i, i, i, p], c_int),
        "sbk_ctc_beam_search_lm_f32": ([p, p, p, i, POINTER(CTCBeamConfig), POINTER(CTCLMTables), p, ctypes.c_size_t, p, p, p,
                                        p, i, i, i, p], c_int),
        "sbk_transducer_greedy_f32": ([POINTER(TransducerWeights), POINTER(TransducerConfig), p, p, p, p, p, p, p, i, i, p],
                                      c_int),
        "sbk_lstm_f32": ([p, p, p, p, p, p, p, i, i, i, p], c_int),
        "sbk_transducer_beam_workspace_bytes": ([POINTER(TransducerWeights), POINTER(TransducerBeamConfig), i, i],
                                                ctypes.c_size_t),
        "sbk_transducer_beam_search_f32": ([POINTER(TransducerWeights), POINTER(TransducerBeamConfig), p, p, ctypes.c_size_t,
                                            p, p, p, p, p, i, i, p], c_int),
        "sbk_transducer_beam_lm_workspace_bytes": ([POINTER(TransducerWeights), POINTER(RNNLMWeights),
                                                    POINTER(TransducerBeamConfig), i, i], ctypes.c_size_t),
        "sbk_transducer_beam_search_lm_f32": ([POINTER(TransducerWeights), POINTER(RNNLMWeights), f,
                                               POINTER(TransducerBeamConfig), p, p, ctypes.c_size_t, p, p, p, p, p, i, i, p],
                                              c_int),
        "sbk_beam_search_workspace_bytes": ([POINTER(DecoderWeights), POINTER(SearchConfig), i, i], ctypes.c_size_t),
        "sbk_beam_search_f32": ([POINTER(DecoderWeights), POINTER(SearchConfig), p, p, p, p, p, ctypes.c_size_t, p, p,
                                 p, p, p, p, p, POINTER(c_int32), i, i, p], c_int),
        "sbk_greedy_search_workspace_bytes": ([POINTER(DecoderWeights), i, i, i], ctypes.c_size_t),
        "sbk_greedy_search_f32": ([POINTER(DecoderWeights), p, p, p, ctypes.c_size_t, p, p, p, POINTER(c_int32), i, i,
                                   i, i, i, i, i, p], c_int),
        "sbk_prompted_greedy_search_workspace_bytes": ([POINTER(DecoderWeights), i, i, i, i], ctypes.c_size_t),
        "sbk_prompted_greedy_search_f32": ([POINTER(DecoderWeights), p, p, p, i, p, p, p, ctypes.c_size_t, p, p, i, i, p, p,
                                            POINTER(c_int32), i, i, i, i, i, p], c_int),
        "sbk_decoder_prefix_workspace_bytes": ([POINTER(DecoderWeights), i, i, i], ctypes.c_size_t),
        "sbk_decoder_prefix_f32": ([POINTER(DecoderWeights), p, p, p, p, ctypes.c_size_t, p, i, i, i, p], c_int),
        "sbk_lm_prefix_workspace_bytes": ([POINTER(LMWeights), i, i], ctypes.c_size_t),
        "sbk_lm_prefix_f32": ([POINTER(LMWeights), p, p, ctypes.c_size_t, p, i, i, p], c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return sig


EXPORTS: tuple = ()
# path -> (CDLL, its exports): ONE object per loaded library for the life of the process.  dlopen hands every load of a path the
# same library (one table of stream workspaces inside it), and _ws_key identifies the library by this object: a second CDLL of
# the same path would register -- and keep -- a second ~134 MB workspace per stream for the same table.
_LIBS: dict = {}


def load(path: Optional[str] = None):
    """Load the HIP library (idempotent).  Raises if it has not been built."""
    global _lib, EXPORTS
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if path not in _LIBS:
        if not os.path.exists(path):
            raise SbkError(
                f"{path} is missing: the MI355X kernels are not built. Run `python -m speechbrain_amd.csrc.build` "
                "(hipcc, gfx950). There is no CPU fallback."
            )
        lib = ctypes.CDLL(path)
        exports = tuple(_declare(lib).keys())
        if lib.sbk_abi_version() != 11:
            raise SbkError(f"ABI version mismatch: {lib.sbk_abi_version()}")
        _LIBS[path] = (lib, exports)
    _lib, EXPORTS = _LIBS[path]
    return _lib


# name -> key of the library's tuning switches (include/sbk.h, enum sbk_knob: SBK_KNOB_<NAME>)
KNOBS = {
    "skinny_off": 2, "cross_rows": 4, "cross_fc256": 8, "tiled_splitk": 14, "sk_mode": 18, "sk_min_rows": 24,
    "x3_route_rows": 34, "x3_route_tiles": 35, "score_fused": 40, "x3r_mode": 41, "x3r_min_rows": 42, "x3r_ln": 45,
    "persist": 47, "persist_grid": 48, "persist_stamps": 49, "x3r_xc": 51, "nt_mask": 53, "self_anc": 55, "x3r_pair": 58,
    "persist_tree": 59, "attn_exp2": 60, "lp256": 61, "x3p_fast_epi": 63,
}


@contextlib.contextmanager
def knobs(**values):
    """``with knobs(persist=0, cross_rows=5): ...`` -- set the named tuning switches for the block and put back what they held
    before, also when the block raises.  The switches are process-wide.  An unknown name raises KeyError before any is set."""
    lib = load()
    wanted = {KNOBS[name]: int(value) for name, value in values.items()}
    found = {key: lib.sbk_prof_get_knob(key) for key in wanted}
    try:
        for key, value in wanted.items():
            lib.sbk_prof_set_knob(key, value)
        yield
    finally:
        for key, value in found.items():
            lib.sbk_prof_set_knob(key, value)


def _chk(rc: int, what: str):
    if rc != 0:
        raise SbkError(f"{what} failed (rc={rc}): {_lib.sbk_last_error().decode()}")


def _dev_ok(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise SbkError(
                "speechbrain_amd ops run on an MI355X (HIP) device only; got a CPU tensor. "
                "Move the module and inputs to 'cuda' (there is no CPU fallback)."
            )
        if not t.is_contiguous():
            raise SbkError("non-contiguous tensor passed to a kernel")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


# The persistent / stream-K kernels need slabs and arrival tickets per stream; the library allocates nothing (include/sbk.h,
# "stream workspace"): the binding registers ONE torch-allocated workspace per (library, device, stream) the first time an
# op is issued on that stream, and keeps it for the life of the process (torch's streams come from a fixed pool and are
# never destroyed).  Every op fetches its stream through _stream(), so no call can reach a kernel without one -- the same
# kernels run on every stream, and a worker stream's first launch allocates nothing inside the library.
_STREAM_WS = {}
_STREAM_WS_LOCK = threading.RLock()
# torch hands out stream HANDLES from a pool (32 per priority): two live Stream objects -- of two transcribers, or a
# transcriber's and ShardedTranscriber's copy stream -- can be the same handle.  An owner that means to release a stream's
# workspace when it retires first RETAINS it; the workspace goes back only when its last owner has released it.
_STREAM_WS_REFS = {}


def _ws_key(stream):
    """(id(lib), device index | "host", handle): the _STREAM_WS key of a torch.cuda.Stream, or (None) of the emulator's NULL one."""
    return (id(load()), stream.device.index, stream.cuda_stream) if stream is not None else (id(load()), "host", 0)


def retain_stream_workspace(stream):
    """Declare an owner of the (device, handle) of ``stream`` (a ConcurrentTranscriber for each of its worker streams)."""
    key = _ws_key(stream)
    with _STREAM_WS_LOCK:
        _STREAM_WS_REFS[key] = _STREAM_WS_REFS.get(key, 0) + 1


class _Workspace:
    """An aligned workspace of exactly ``nbytes`` for one library call: ``ptr`` is the address the entry gets, ``buf`` the uint8
    tensor that owns it, ``off`` the aligned start inside ``buf``.  A fresh allocation of max(nbytes, floor) + align bytes, or
    -- ``per_stream`` -- the grow-only search buffer of the current stream (_search_workspace), held for the ``with`` block."""
    __slots__ = ("buf", "off", "ptr", "key")

    def __init__(self, nbytes, device, align=256, floor=0, per_stream=False):
        size = max(nbytes, floor) + align
        self.buf, self.key = (_search_workspace(size, device) if per_stream
                              else (torch.empty(size, dtype=torch.uint8, device=device), None))
        self.off = (-self.buf.data_ptr()) % align
        self.ptr = c_void_p(self.buf.data_ptr() + self.off)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _search_workspace_done(self.key)


def _register_workspace(key, device, handle):
    lib = load()
    with _STREAM_WS_LOCK:
        if key in _STREAM_WS:
            return
        nbytes = lib.sbk_stream_workspace_bytes()
        ws = _Workspace(nbytes, device)
        # the library keys its table on hipGetDevice(): make the tensor's device the current one for the call
        ctx = torch.cuda.device(device) if getattr(device, "type", None) == "cuda" else contextlib.nullcontext()
        with ctx:
            _chk(lib.sbk_stream_workspace_set(c_void_p(handle) if handle is not None else None, ws.ptr, nbytes),
                 "sbk_stream_workspace_set")
        _STREAM_WS[key] = ws


def forget_stream_owner(stream):
    """An owner of ``stream`` went away WITHOUT releasing (a transcriber dropped without ``close()``): its claim is withdrawn, the
    workspace stays registered -- the handle's next owner releases it, or it lives as long as the process (one per pooled handle)."""
    key = _ws_key(stream)
    with _STREAM_WS_LOCK:
        left = _STREAM_WS_REFS.get(key, 0) - 1
        if left > 0:
            _STREAM_WS_REFS[key] = left
        else:
            _STREAM_WS_REFS.pop(key, None)


def release_stream_workspace(stream) -> bool:
    """Give back the workspace registered for a ``torch.cuda.Stream`` that will not be used again (a worker stream of a
    ConcurrentTranscriber that is being closed): sbk_stream_workspace_release, then the ~134 MB return to torch's allocator once
    the stream has drained.  Streams that never issued an op have none (False)."""
    lib = load()
    key = _ws_key(stream)
    with _STREAM_WS_LOCK:
        left = _STREAM_WS_REFS.get(key, 0) - 1
        if left > 0:  # another live owner of the same pooled handle: it keeps the workspace
            _STREAM_WS_REFS[key] = left
            return False
        _STREAM_WS_REFS.pop(key, None)
        if key not in _STREAM_WS:
            return False
    stream.synchronize()  # (outside the lock: other streams' first launches register their workspaces meanwhile)
    with _STREAM_WS_LOCK:
        if _STREAM_WS_REFS.get(key, 0) > 0:  # (retained again while the stream drained)
            return False
        ws = _STREAM_WS.pop(key, None)
        if ws is None:
            return False
        with torch.cuda.device(stream.device):
            _chk(lib.sbk_stream_workspace_release(c_void_p(stream.cuda_stream)), "sbk_stream_workspace_release")
    return True


def _stream(t: torch.Tensor):
    # (host tensors only reach a kernel under the test emulator: its one "stream" is NULL)
    cur = torch.cuda.current_stream(t.device) if t.is_cuda else None
    key = _ws_key(cur)
    if key not in _STREAM_WS:
        _register_workspace(key, t.device, cur.cuda_stream if cur is not None else None)
    return c_void_p(cur.cuda_stream) if cur is not None else None


def _f32(t):
    if t.dtype != torch.float32:
        raise SbkError(f"expected float32, got {t.dtype}")
    return t


# ------------------------------------------------------------------ precision of the dense contractions
_tls = threading.local()


def precision() -> str:
    """"fp32" (parity path, default) or an opt-in reduced-precision operand type for the large GEMMs, all with fp32
    accumulation: "bf16" (also the bf16 attention kernel), "fp16", "fp8" (e4m3, per-tensor scales)."""
    return getattr(_tls, "precision", "fp32")


@contextlib.contextmanager
def precision_scope(p):
    """Per host thread (the batches in flight of ConcurrentTranscriber each carry their own)."""
    p = p or "fp32"
    if p not in ("fp32", "bf16", "fp16", "fp8"):
        raise NotImplementedError(f"precision {p!r}: 'fp32' (parity) or the opt-in 'bf16' / 'fp16' / 'fp8' GEMM operands")
    old = precision()
    _tls.precision = p
    try:
        yield
    finally:
        _tls.precision = old


# fp32 contractions with many rows (the encoder's) run on the bf16 matrix pipe through the exact three-way operand split
# (sbk_gemm_nt_f32x3, include/sbk.h): the same fp32 result class at 2-3x the rate of the fp32 MFMA kernels.  "0" keeps
# every contraction on v_mfma_f32_32x32x2_f32 (A/B runs, tests of the fp32-MFMA kernels).
F32X3 = os.environ.get("SBK_F32X3", "1") != "0"
F32X3_MIN_ROWS = int(os.environ.get("SBK_F32X3_MIN_ROWS", "2048"))
F32X3_MIN_TILES = int(os.environ.get("SBK_F32X3_MIN_TILES", "192"))
# ... and, with the activation operand pre-split as well, through sbk_gemm_nt_x3p (csrc/gemm_x3p.hip: 256-wide tiles)
X3P = os.environ.get("SBK_X3P", "1") != "0"
# the decode step's few-row projections on the bf16 matrix pipe (sbk_gemm_nt_x3r: panel images of the decoder's weights)
X3R = os.environ.get("SBK_X3R", "1") != "0"
X3P_MIN_TILES = int(os.environ.get("SBK_X3P_MIN_TILES", "96"))


def _x3_shape(N: int, K: int) -> bool:
    """Weights [N, K] that have an "x3" image (sbk_split_bf16x3: 32-deep K groups, rows moved four at a time)."""
    return K % 32 == 0 and K >= 64 and N % 4 == 0


def f32x3_ok(M: int, K: int, w: torch.Tensor) -> bool:
    """Shapes routed to sbk_gemm_nt_f32x3.  Measured on MI355X (tools/microbench.py --x3, profiles/r03_f32x3_sweep.log):
    from ~0.75 tiles of 128 x 128 per CU on the split-operand kernel wins (M = 8 000, N = 512: 38.9 vs 43.2 us); below, the
    fp32-MFMA tile kernels do (M = 4 032, N = 512: 25.4 vs 30.6 us)."""
    if not (F32X3 and M >= F32X3_MIN_ROWS and w.dim() == 2 and w.is_contiguous() and _x3_shape(w.shape[0], K)):
        return False
    return ((M + 127) // 128) * ((w.shape[0] + 127) // 128) >= F32X3_MIN_TILES


def _aligned16(*ts) -> bool:
    """(the split-operand kernel moves rows of C / residual / bias as 16-byte vectors)"""
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


# ------------------------------------------------------------------ ops
def _rows(a, w, residual=None):
    """The GEMM wrappers' view of their operands: (a as rows [M, K], residual as rows [M, N] or None, M, N, K)."""
    K, N = a.shape[-1], w.shape[0]
    a2 = a.reshape(-1, K)
    return a2, (residual.reshape(-1, N) if residual is not None else None), a2.shape[0], N, K


def gemm_nt(a: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE, alpha=1.0, out=None,
            seq_len=None, rows_per_seq=0):
    """out[M,N] = residual + alpha * act(a[M,K] @ w[N,K]^T + bias).  `a` may have leading dims.

    With ``seq_len`` (int32 [batch]) rows are [batch][rows_per_seq] and the rows past each
    sequence's length contribute 0 before the residual is added."""
    lib = load()
    if isinstance(a, Panel):  # the producer wrote the operand's panel image (layernorm_x3p, gemm_nt_x3p(panel_out=True))
        return gemm_nt_x3p(a, w, bias, residual, act, alpha, out=out, seq_len=seq_len, rows_per_seq=rows_per_seq)
    a2, r2, M, N, K = _rows(a, w, residual)
    if precision() != "fp32" and M >= 256 and K % (16 if precision() == "fp8" else 8) == 0 and w.is_contiguous():
        return gemm_nt_bf16(a, w, bias, residual, act, alpha, seq_len, rows_per_seq, out=out, kind=precision())  # opt-in fast path
    _dev_ok(a2, w, bias, residual)
    _f32(a2), _f32(w)
    if out is None:
        out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    _dev_ok(seq_len)
    if x3p_ok(M, K, w) and _aligned16(a2, out, bias, r2):  # both operands pre-split, 256-wide tiles (csrc/gemm_x3p.hip)
        return gemm_nt_x3p(split_x3p(a2), w, bias, r2, act, alpha, out=out, seq_len=seq_len, rows_per_seq=rows_per_seq)
    if f32x3_ok(M, K, w) and _aligned16(a2, out, bias, r2):
        _chk(lib.sbk_gemm_nt_f32x3(_p(a2), K, _p(lp_weight(w, "x3")), _p(bias), _p(r2), N, _p(out), N, M, N, K, act,
                                   float(alpha), _p(seq_len), int(rows_per_seq), _stream(a2)), "sbk_gemm_nt_f32x3")
        return out
    _chk(lib.sbk_gemm_nt_f32(_p(a2), K, _p(w), w.stride(0), _p(bias), _p(r2), N, _p(out), N, M, N, K, act,
                             float(alpha), _p(seq_len), int(rows_per_seq), _stream(a2)), "sbk_gemm_nt_f32")
    return out


def gemm_nt_rows(a_flat: torch.Tensor, M: int, K: int, lda: int, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE,
                 alpha=1.0, out=None):
    """gemm_nt whose A operand is M rows of K floats starting every ``lda`` floats in the flat tensor ``a_flat``.
    ``lda`` < K makes consecutive rows overlap: a strided window over a time-major signal, i.e. a 1-D convolution read
    in place (no im2col copy).  out [M,N] (contiguous)."""
    lib = load()
    N = w.shape[0]
    if M == 0:
        return out if out is not None else torch.empty(0, N, dtype=torch.float32, device=a_flat.device)
    if a_flat.dim() != 1 or a_flat.numel() < (M - 1) * lda + K or w.shape[1] != K:
        raise SbkError(f"gemm_nt_rows: {M} rows of {K} every {lda} do not fit {tuple(a_flat.shape)} / {tuple(w.shape)}")
    _dev_ok(a_flat, w, bias, residual, out)
    _f32(a_flat), _f32(w)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a_flat.device)
    # (precision "fp8" with fp8 activations: the sliding-window operand stays fp32 in memory, so the two convolutions of the
    # Whisper front-end take the bf16-operand kernel there too -- 2 % of the encoder's flops)
    if (precision() == "bf16" or (precision() == "fp8" and FP8_ACTIVATIONS)) and M >= 256 and K % 8 == 0 and lda % 4 == 0:
        _chk(lib.sbk_gemm_nt_bf16(_p(a_flat), int(lda), _p(bf16_weight(w)), K, _p(bias), _p(residual), N, _p(out), N, M, N, K,
                                  act, float(alpha), None, 0, _stream(a_flat)), "sbk_gemm_nt_bf16")
        return out
    if x3p_ok(M, K, w) and _aligned16(out, bias, residual):
        return gemm_nt_x3p(split_x3p(a_flat, rows=M, K=K, ldx=lda), w, bias, residual, act, alpha, out=out)
    if f32x3_ok(M, K, w) and lda % 4 == 0 and _aligned16(a_flat, out, bias, residual):
        _chk(lib.sbk_gemm_nt_f32x3(_p(a_flat), int(lda), _p(lp_weight(w, "x3")), _p(bias), _p(residual), N, _p(out), N, M, N, K,
                                   act, float(alpha), None, 0, _stream(a_flat)), "sbk_gemm_nt_f32x3")
        return out
    _chk(lib.sbk_gemm_nt_f32(_p(a_flat), int(lda), _p(w), w.stride(0), _p(bias), _p(residual), N, _p(out), N, M, N, K, act,
                             float(alpha), None, 0, _stream(a_flat)), "sbk_gemm_nt_f32")
    return out


# ------------------------------------------------------------------ both operands pre-split, panel layout (csrc/gemm_x3p.hip)
class Panel:
    """The panel image (include/sbk.h, sbk_split_x3p) of an fp32 matrix [rows, K]: the A operand of sbk_gemm_nt_x3p."""
    __slots__ = ("data", "rows", "K", "lead")

    def __init__(self, data, rows, K, lead=None):
        self.data, self.rows, self.K, self.lead = data, rows, K, lead  # lead: leading dims of the activation it stands for

    @property
    def device(self):
        return self.data.device

    # what a consumer written for the fp32 activation asks of its operand (RoPEMHA.core / the *_group cores: ADVICE r4)
    @property
    def shape(self):
        return torch.Size((tuple(self.lead) if self.lead is not None else (self.rows,)) + (self.K,))

    @property
    def dtype(self):
        return torch.float32

    def new_empty_rows(self) -> torch.Tensor:
        """An fp32 tensor of the shape of the activation this image stands for (``torch.empty_like`` of a tensor operand)."""
        return torch.empty(self.shape, dtype=torch.float32, device=self.data.device)


def panel_empty(rows: int, K: int, device, lead=None) -> Panel:
    n = ((rows + 63) // 64) * 64 * K * 3  # int16 elements
    return Panel(torch.empty(n, dtype=torch.int16, device=device), rows, K, lead)


def split_x3p(x: torch.Tensor, rows: Optional[int] = None, K: Optional[int] = None, ldx: Optional[int] = None) -> Panel:
    """x [..., K] fp32 (contiguous) -> its panel image; with rows / K / ldx: `rows` windows of K floats every ldx floats of
    the flat tensor x (gemm_nt_rows' sliding-window operand)."""
    lib = load()
    _dev_ok(x)
    _f32(x)
    lead = None
    if rows is None:
        K = x.shape[-1]
        lead = tuple(x.shape[:-1])
        x = x.reshape(-1, K)
        rows, ldx = x.shape[0], K
    out = panel_empty(rows, K, x.device, lead)
    _chk(lib.sbk_split_x3p(_p(x), int(ldx), _p(out.data), rows, K, _stream(x)), "sbk_split_x3p")
    return out


def panel_for(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when the contraction x[..., K] @ w^T takes the both-operands-pre-split route on the fp32 path, i.e. when the
    kernel that PRODUCES x should write it as a Panel (layernorm_x3p, gemm_nt_x3p(panel_out=True)) instead of fp32."""
    K = x.shape[-1] if not isinstance(x, Panel) else x.K
    M = (x.numel() // K) if not isinstance(x, Panel) else x.rows
    return precision() == "fp32" and x3p_ok(M, K, w)


def layernorm_x3p(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act=ACT_NONE) -> Panel:
    """``layernorm`` written directly as the panel image of its result (sbk_layernorm_x3p): the A operand of the
    gemm_nt that follows, without the fp32 round trip and the split pass."""
    lib = load()
    d = gamma.numel()
    x2 = x.reshape(-1, d)
    _dev_ok(x2, gamma, beta)
    _f32(x2)
    out = panel_empty(x2.shape[0], d, x.device, tuple(x.shape[:-1]))
    _chk(lib.sbk_layernorm_x3p(_p(x2), _p(gamma), _p(beta), _p(out.data), x2.shape[0], d, float(eps), act, _stream(x2)),
         "sbk_layernorm_x3p")
    return out


def x3p_ok(M: int, K: int, w: torch.Tensor) -> bool:
    """Shapes routed to sbk_gemm_nt_x3p: from F32X3_MIN_ROWS rows on, K % 16 == 0, and enough 256 x 128 tiles to give most
    CUs one (tools/microbench.py --x3p)."""
    if not (F32X3 and X3P and M >= F32X3_MIN_ROWS and K % 16 == 0 and K >= 32 and w.dim() == 2 and w.is_contiguous()):
        return False
    return w.shape[0] % 4 == 0 and ((M + 255) // 256) * ((w.shape[0] + 127) // 128) >= X3P_MIN_TILES


def gemm_nt_x3p(a: Panel, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE, alpha=1.0, out=None, seq_len=None,
                rows_per_seq=0, panel_out=False, fp32_out=True):
    """out[M,N] = residual + alpha * act(A @ w^T + bias) with A given as its panel image.  ``panel_out``: also (or, with
    ``fp32_out=False``, only) return the result as a Panel -- the A operand of the next contraction."""
    lib = load()
    M, K, N = a.rows, a.K, w.shape[0]
    _dev_ok(a.data, w, bias, residual, seq_len)
    wp = lp_weight(w, "x3p")
    lead = a.lead if a.lead is not None else (M,)
    if fp32_out and out is None:
        out = torch.empty(*lead, N, dtype=torch.float32, device=a.device)
    r2 = residual.reshape(-1, N) if residual is not None else None
    pc = panel_empty(M, N, a.device, lead) if panel_out else None
    # The kernel moves rows of C / residual / bias as 16-byte vectors.  A tensor operand falls back to another kernel in
    # gemm_nt; a Panel operand has no fp32 form to fall back with, so unaligned views go through aligned temporaries
    # (fresh torch allocations are 512-byte aligned) -- ADVICE r4
    user_out = None
    if bias is not None and bias.data_ptr() % 16:
        bias = bias.clone()
    if r2 is not None and r2.data_ptr() % 16:
        r2 = r2.clone()
    if fp32_out and out.data_ptr() % 16:
        user_out, out = out, torch.empty(out.shape, dtype=torch.float32, device=out.device)
    _chk(lib.sbk_gemm_nt_x3p(_p(a.data), _p(wp), _p(bias), _p(r2), N, _p(out) if fp32_out else None, N,
                             _p(pc.data) if pc is not None else None, M, N, K, act, float(alpha), _p(seq_len), int(rows_per_seq),
                             _stream(a.data)), "sbk_gemm_nt_x3p")
    if user_out is not None:
        user_out.copy_(out)
        out = user_out
    if panel_out:
        return (out, pc) if fp32_out else pc
    return out


def gemm_nt_x3r(a: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE, alpha=1.0):
    """out[M,N] = residual + alpha * act(a @ w^T + bias) for FEW rows (a decoding step's projections) on the bf16 matrix
    pipe (sbk_gemm_nt_x3r): ``a`` fp32 (split in registers), ``w`` is used through its cached panel image."""
    lib = load()
    a2, r2, M, N, K = _rows(a, w, residual)
    _dev_ok(a2, w, bias, residual)
    _f32(a2)
    out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    _chk(lib.sbk_gemm_nt_x3r(_p(a2), K, _p(lp_weight(w, "x3p")), _p(bias), _p(r2), N, _p(out), N, M, N, K, act, float(alpha),
                             _stream(w)), "sbk_gemm_nt_x3r")
    return out


def gemm_ln_nt_x3r(a: torch.Tensor, wf: torch.Tensor, bf, eps, residual=None, act=ACT_NONE, alpha=1.0):
    """residual + alpha * act(LN(a) @ W^T + b) for FEW rows on the bf16 matrix pipe, the LayerNorm in the projection's
    prologue (sbk_gemm_ln_nt_x3r): gamma / beta pre-folded into (wf, bf) as for ``gemm_ln_nt``; ``wf`` is used through its
    cached panel image.  K = 256, 512, 1024 or 1280."""
    lib = load()
    a2, r2, M, N, K = _rows(a, wf, residual)
    _dev_ok(a2, wf, bf, residual)
    _f32(a2)
    out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    _chk(lib.sbk_gemm_ln_nt_x3r(_p(a2), K, _p(lp_weight(wf, "x3p")), _p(bf), _p(r2), N, _p(out), N, M, N, K,
                                float(eps), act, float(alpha), _stream(wf)), "sbk_gemm_ln_nt_x3r")
    return out


class _Ready:
    """A derived weight image (bf16 / x3 copy, LayerNorm-folded projection, a handle's tables) is produced by kernels on
    the stream of the thread that first asked for it; the batches in flight run on other streams and may ask for it a
    few microseconds later.  The producer records an event; a consumer on another stream waits for it (on the
    device, not on the host) until it has completed once."""
    __slots__ = ("ev", "sid")

    def __init__(self, device):
        self.ev, self.sid = None, 0
        if device.type == "cuda":
            cur = torch.cuda.current_stream(device)
            self.ev = torch.cuda.Event()
            self.ev.record(cur)
            self.sid = cur.cuda_stream

    def wait(self, device):
        ev = self.ev
        if ev is None:
            return
        if ev.query():
            self.ev = None  # (benign race: the event has completed for everybody)
            return
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream != self.sid:
            cur.wait_event(ev)


def source_key(sources, extra=()):
    """The validity key of what is derived from the tensors ``sources``: ``extra`` + (data_ptr, _version, device) of each.  An
    in-place update (load_state_dict, copy_) bumps _version; ``param.data = other`` (nn.Module._apply) changes data_ptr."""
    return tuple(extra) + tuple((t.data_ptr(), t._version, t.device) for t in sources if t is not None)


_DERIVED_LOCK = threading.RLock()  # (re-entrant, as _BF16_LOCK below: a build allocates, and may build another Derived)
_Hit = collections.namedtuple("_Hit", "key value ready device")  # (what a Derived holds; ready: the producer's _Ready)


class Derived:
    """One value derived from parameter tensors (a permuted / stacked / folded copy, a TransducerPrepared), owned by the module
    that uses it and shared by its shallow copies (the per-worker searchers of a ConcurrentTranscriber): built once per
    ``source_key``, by one thread, and handed to the other streams through its producer's event (_Ready)."""
    __slots__ = ("_hit",)

    def __init__(self):
        self._hit = None  # (a _Hit, published as one object: a hit takes no lock)

    def __deepcopy__(self, memo):
        return Derived()

    def get(self, sources, build, device=None, extra=()):
        """The value ``build()`` returned for these ``sources`` (parameter tensors, None entries skipped) and ``extra``; built
        under torch.no_grad() on a miss.  ``device``: where the value lives (default: the first source's)."""
        key = source_key(sources, extra)
        hit = self._hit
        if hit is None or hit.key != key:
            with _DERIVED_LOCK:
                hit = self._hit
                if hit is None or hit.key != key:
                    self._hit = None  # (a build that raises leaves nothing behind)
                    device = device if device is not None else next(t for t in sources if t is not None).device
                    with torch.no_grad():
                        value = build()
                    hit = self._hit = _Hit(key, value, _Ready(device), device)
        hit.ready.wait(hit.device)  # (made on another worker's stream a moment ago?)
        return hit.value


# (an entry of _BF16_WEIGHTS; ref: weak reference to the base tensor; scale: "fp8" float, "fp8r" tensor [N], else None)
_Image = collections.namedtuple("_Image", "ref version image scale ready data_ptr")
_BF16_WEIGHTS = {}  # (id(base tensor), kind, view geometry) -> _Image
# re-entrant: the weak-reference callback below takes the lock too, and a cyclic-GC pass started by an allocation INSIDE a
# locked region may run it on the thread that already holds the lock
_BF16_LOCK = threading.RLock()


def _make_image(w: torch.Tensor, kind: str):
    """(image, scale) of the fp32 matrix ``w`` for ``kind`` (see lp_weight), written on the current stream."""
    lib = load()
    w2 = w.detach().contiguous()
    _dev_ok(w2)
    _f32(w2)
    scale = None
    if kind == "fp8":
        scale = max(float(w2.abs().max()), 1e-30) / 448.0  # (once per weight: a host round trip at load time)
        out = torch.empty(w2.shape, dtype=torch.uint8, device=w.device)
        _chk(lib.sbk_f32_to_fp8(_p(w2), _p(out), w2.numel(), 1.0 / scale, _stream(w2)), "sbk_f32_to_fp8")
    elif kind == "fp8r":  # e4m3 with one scale per output channel (sbk_quant_rows_fp8): the W operand of gemm_nt_fp8a
        out = torch.empty(w2.shape, dtype=torch.uint8, device=w.device)
        scale = torch.empty(w2.shape[0], dtype=torch.float32, device=w.device)
        _chk(lib.sbk_quant_rows_fp8(_p(w2), w2.shape[1], _p(out), _p(scale), w2.shape[0], w2.shape[1], _stream(w2)), "sbk_quant_rows_fp8")
    elif kind == "x3":
        N, K = w2.shape
        out = torch.empty(N, K // 32, 3, 32, dtype=torch.int16, device=w.device)
        _chk(lib.sbk_split_bf16x3(_p(w2), K, _p(out), N, K, _stream(w2)), "sbk_split_bf16x3")
    elif kind == "x3p":
        N, K = w2.shape
        out = torch.empty(((N + 63) // 64) * 64 * K * 3, dtype=torch.int16, device=w.device)
        _chk(lib.sbk_split_x3p(_p(w2), K, _p(out), N, K, _stream(w2)), "sbk_split_x3p")
    else:
        out = torch.empty(w2.shape, dtype=torch.int16, device=w.device)
        fn = lib.sbk_f32_to_bf16 if kind == "bf16" else lib.sbk_f32_to_f16
        _chk(fn(_p(w2), _p(out), w2.numel(), _stream(w2)), "sbk_f32_to_" + kind)
    return out, scale


def lp_weight(w: torch.Tensor, kind: str = "bf16"):
    """The reduced-precision image of a weight matrix ("bf16" / "fp16": int16 bits; "fp8": (uint8 e4m3 bits, w_scale);
    "x3": the exact three-piece bf16 split [N, K/32, 3, 32] of sbk_split_bf16x3 -- not reduced: the pieces sum to w),
    cached for the lifetime of THAT tensor object: the entry holds a weak reference to its source and is used only while
    ``ref() is w`` and the version counter is unchanged (a freed model's addresses are commonly handed to the next
    model of the same shapes by the caching allocator, and load_state_dict leaves ``_version`` alike -- a (data_ptr,
    version, shape) key would then serve the OLD model's weights).  Entries die with their tensor (weakref callback);
    insert / evict under a lock (worker threads)."""
    # a VIEW of a parameter (conv weight [2d,d,1] reshaped to [2d,d], a slice of a stacked projection) is a new tensor object
    # on every call: the entry belongs to the view's base and the view's geometry, so the image is made once
    base = w._base if w._base is not None else w
    key = (id(base), kind, w.storage_offset(), tuple(w.shape), tuple(w.stride()))
    with _BF16_LOCK:
        hit = _BF16_WEIGHTS.get(key)
        # (data_ptr: `param.data = other` -- nn.Module._apply, a manual weight swap -- keeps the object and its version)
        if (hit is not None and hit.ref() is base and hit.version == w._version and hit.image.device == w.device
                and hit.data_ptr == w.data_ptr()):
            hit.ready.wait(w.device)  # (made on another worker's stream a moment ago?)
            return hit.image if kind not in ("fp8", "fp8r") else (hit.image, hit.scale)
    out, scale = _make_image(w, kind)

    def _drop(_ref, key=key):
        with _BF16_LOCK:
            cur = _BF16_WEIGHTS.get(key)
            if cur is not None and cur.ref is _ref:
                del _BF16_WEIGHTS[key]

    with _BF16_LOCK:
        _BF16_WEIGHTS[key] = _Image(weakref.ref(base, _drop), w._version, out, scale, _Ready(w.device), w.data_ptr())
    return out if kind not in ("fp8", "fp8r") else (out, scale)


def bf16_weight(w: torch.Tensor) -> torch.Tensor:
    return lp_weight(w, "bf16")


def gemm_nt_bf16(a: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE, alpha=1.0, seq_len=None,
                 rows_per_seq=0, out=None, kind="bf16"):
    """gemm_nt with reduced-precision operands / fp32 accumulation (opt-in fast path; `w` is the fp32 parameter, its
    image of ``kind`` -- "bf16", "fp16" or "fp8" (e4m3 with per-tensor scales: the weight's at conversion time, the
    activation's max |a| computed on the device per call) -- is cached).  Falls back to the fp32 kernel for shapes the
    kernels do not take (K % 8 != 0; fp8: K % 16 != 0)."""
    K = a.shape[-1]
    if K % (16 if kind == "fp8" else 8) != 0:
        with precision_scope("fp32"):
            return gemm_nt(a, w, bias, residual, act, alpha, out=out, seq_len=seq_len, rows_per_seq=rows_per_seq)
    lib = load()
    a2, r2, M, N, K = _rows(a, w, residual)
    _dev_ok(a2, bias, residual, seq_len)
    _f32(a2)
    if out is None:
        out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    if kind == "fp8":
        wq, w_scale = lp_weight(w, "fp8")
        amax = torch.empty(1, dtype=torch.float32, device=a.device)
        _chk(lib.sbk_absmax_f32(_p(a2), a2.numel(), _p(amax), _stream(a2)), "sbk_absmax_f32")
        _chk(lib.sbk_gemm_nt_fp8(_p(a2), K, _p(amax), _p(wq), K, float(w_scale), _p(bias), _p(r2), N, _p(out), N, M, N, K,
                                 act, float(alpha), _p(seq_len), int(rows_per_seq), _stream(a2)), "sbk_gemm_nt_fp8")
        return out
    wb = lp_weight(w, kind)
    fn = lib.sbk_gemm_nt_bf16 if kind == "bf16" else lib.sbk_gemm_nt_f16
    _chk(fn(_p(a2), K, _p(wb), K, _p(bias), _p(r2), N, _p(out), N, M, N, K, act, float(alpha),
            _p(seq_len), int(rows_per_seq), _stream(a2)), "sbk_gemm_nt_" + kind)
    return out


# precision "bf16": keep the operands of consecutive contractions in bf16 in memory where a model's forward supports it
# (the Whisper encoder); False = every contraction reads fp32 activations and rounds them on load (A/B, tests)
BF16_ACTIVATIONS = os.environ.get("SBK_BF16_ACTIVATIONS", "1") != "0"
# rows from which the Conformer feed-forward pairs take that path.  Measured on MI355X: one stream, 32 x 20 s (16 000 rows)
# encodes in 15.7 instead of 17.0 ms, 32 x 10 s in 9.4 instead of 8.9 (tools/microbench.py --enc-bf16,
# profiles/r03_bf16_attention_lds_and_conformer_bf16.log); the eight-worker job of bench.py --precision bf16 runs at
# 12 093 audio-s/s with every batch on this path, 11 752 from 16 000 rows, 11 887 without (profiles/r03_bf16_bench_leg_ab.log)
BF16A_MIN_ROWS = int(os.environ.get("SBK_BF16A_MIN_ROWS", "256"))


def bf16a_ok(K: int) -> bool:
    """Shapes the bf16-activation contraction (sbk_gemm_nt_bf16a) takes: K a multiple of its 64-deep K tile."""
    return K % 64 == 0


def gemm_nt_bf16a(a: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE, alpha=1.0,
                  out_dtype=torch.float32):
    """epilogue(a . w^T) with ``a`` ALREADY bf16 in memory (torch.bfloat16 [..., K], written by layernorm_bf16 /
    rope_attention(out_dtype=bf16) / a previous gemm_nt_bf16a) and the cached bf16 image of the fp32 parameter ``w``;
    fp32 accumulation, fp32 residual; the result is fp32 or -- ``out_dtype=torch.bfloat16`` -- the next contraction's
    bf16 operand."""
    lib = load()
    a2, r2, M, N, K = _rows(a, w, residual)
    _dev_ok(a2, bias, residual)
    if a2.dtype != torch.bfloat16 or not a2.is_contiguous():
        raise SbkError("gemm_nt_bf16a: the activation operand must be a contiguous torch.bfloat16 tensor")
    wb = lp_weight(w, "bf16")
    out = torch.empty(*a.shape[:-1], N, dtype=out_dtype, device=a.device)
    c32, cb = (out, None) if out_dtype == torch.float32 else (None, out)
    _chk(lib.sbk_gemm_nt_bf16a(_p(a2), K, _p(wb), K, _p(bias), _p(r2), N, _p(c32), N, _p(cb), N, M, N, K, act,
                               float(alpha), _stream(a2)), "sbk_gemm_nt_bf16a")
    return out


def layernorm_bf16(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act=ACT_NONE):
    """``layernorm`` written as bf16 (round to nearest even): the operand of a following gemm_nt_bf16a."""
    lib = load()
    d = gamma.numel()
    x2 = x.reshape(-1, d)
    _dev_ok(x2, gamma, beta)
    _f32(x2)
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _chk(lib.sbk_layernorm_bf16o(_p(x2), _p(gamma), _p(beta), _p(out), x2.shape[0], d, float(eps), act, _stream(x2)),
         "sbk_layernorm_bf16o")
    return out


# precision "fp8": fp8 (e4m3) activations between the contractions of the Whisper encoder, one fp32 scale per row, on the
# 2 x-rate fp8 matrix instruction (sbk_gemm_nt_fp8a); False = the round-3 path (fp32 activations, per-tensor scales)
FP8_ACTIVATIONS = os.environ.get("SBK_FP8_ACTIVATIONS", "1") != "0"


class Fp8Rows:
    """An activation as e4m3 bytes with one fp32 scale per row (scale None: 1): value = scale[row] * e4m3."""
    __slots__ = ("q", "scale")

    def __init__(self, q, scale):
        self.q, self.scale = q, scale

    @property
    def shape(self):
        return self.q.shape


def fp8a_ok(K: int) -> bool:
    """Shapes the fp8-activation contraction (sbk_gemm_nt_fp8a) takes: K a multiple of its 128-deep K tile."""
    return K % 128 == 0


def layernorm_fp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act=ACT_NONE) -> Fp8Rows:
    """``layernorm`` written as e4m3 rows with one scale per row (row maximum / 448): the operand of gemm_nt_fp8a."""
    lib = load()
    d = gamma.numel()
    x2 = x.reshape(-1, d)
    _dev_ok(x2, gamma, beta)
    _f32(x2)
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    scale = torch.empty(x2.shape[0], dtype=torch.float32, device=x.device)
    _chk(lib.sbk_layernorm_fp8o(_p(x2), _p(gamma), _p(beta), _p(q), _p(scale), x2.shape[0], d, float(eps), act, _stream(x2)),
         "sbk_layernorm_fp8o")
    return Fp8Rows(q, scale)


def quant_rows_fp8(x: torch.Tensor) -> Fp8Rows:
    """x [..., d] fp32 or bf16 -> e4m3 rows with one scale per row."""
    lib = load()
    d = x.shape[-1]
    x2 = x.reshape(-1, d).contiguous()
    _dev_ok(x2)
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    scale = torch.empty(x2.shape[0], dtype=torch.float32, device=x.device)
    if x2.dtype == torch.bfloat16:
        _chk(lib.sbk_quant_rows_bf16_fp8(_p(x2), d, _p(q), _p(scale), x2.shape[0], d, _stream(x2)), "sbk_quant_rows_bf16_fp8")
    else:
        _f32(x2)
        _chk(lib.sbk_quant_rows_fp8(_p(x2), d, _p(q), _p(scale), x2.shape[0], d, _stream(x2)), "sbk_quant_rows_fp8")
    return Fp8Rows(q, scale)


def gemm_nt_fp8a(a: Fp8Rows, w: torch.Tensor, bias=None, residual=None, act=ACT_NONE, alpha=1.0, out_dtype=torch.float32):
    """epilogue(a . w^T) with ``a`` ALREADY fp8 in memory (layernorm_fp8 / quant_rows_fp8 / a previous call's fp8 output) and
    the cached per-channel-scaled e4m3 image of the fp32 parameter ``w``; fp32 accumulation, fp32 residual.  The result is
    fp32, torch.bfloat16 (the attention kernel's operand) or -- ``out_dtype="fp8"`` -- e4m3 at scale 1 (an Fp8Rows
    without scales: the hidden layer of a feed-forward pair)."""
    lib = load()
    a2, r2, M, N, K = _rows(a.q, w, residual)
    _dev_ok(a2, a.scale, bias, residual)
    wq, w_scale = lp_weight(w, "fp8r")
    lead = tuple(a.q.shape[:-1])
    c = cb = c8 = None
    if out_dtype == "fp8":
        c8 = torch.empty(*lead, N, dtype=torch.uint8, device=a2.device)
    elif out_dtype == torch.bfloat16:
        cb = torch.empty(*lead, N, dtype=torch.bfloat16, device=a2.device)
    else:
        c = torch.empty(*lead, N, dtype=torch.float32, device=a2.device)
    _chk(lib.sbk_gemm_nt_fp8a(_p(a2), K, _p(a.scale), _p(wq), K, _p(w_scale), _p(bias), _p(r2), N, _p(c), N, _p(cb), N,
                              _p(c8), N, 1.0, M, N, K, act, float(alpha), _stream(a2)), "sbk_gemm_nt_fp8a")
    if c8 is not None:
        return Fp8Rows(c8, None)
    return cb if cb is not None else c


def gemm_nt_splitk(a, w, bias=None, residual=None, act=ACT_NONE, alpha=1.0, slices=8):
    """gemm_nt for few-row operands with a caller-provided split-K workspace."""
    lib = load()
    a2, r2, M, N, K = _rows(a, w, residual)
    _dev_ok(a2, w, bias, residual)
    out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(1, slices * M * N), dtype=torch.float32, device=a.device)
    _chk(lib.sbk_gemm_nt_splitk_f32(_p(a2), K, _p(w), w.stride(0), _p(bias), _p(r2), N, _p(out), N, M, N, K, act,
                                    float(alpha), _p(ws), ws.numel(), _stream(a2)), "sbk_gemm_nt_splitk_f32")
    return out


def gemm_ln_nt(a, wf, bf, eps, residual=None, act=ACT_NONE, alpha=1.0):
    """LN(a) @ W^T + b with gamma/beta pre-folded into (wf, bf) (see include/sbk.h)."""
    lib = load()
    a2, r2, M, N, K = _rows(a, wf, residual)
    _dev_ok(a2, wf, bf, residual)
    out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    _chk(lib.sbk_gemm_ln_nt_f32(_p(a2), K, _p(wf), K, _p(bf), _p(r2), N, _p(out), N, M, N, K, float(eps), act,
                                float(alpha), _stream(a2)), "sbk_gemm_ln_nt_f32")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act=ACT_NONE, out=None):
    """LayerNorm over the trailing gamma.numel() elements of every row."""
    lib = load()
    d = gamma.numel()
    x2 = x.reshape(-1, d)
    _dev_ok(x2, gamma, beta)
    _f32(x2)
    if out is None:
        out = torch.empty_like(x)
    _chk(lib.sbk_layernorm_f32(_p(x2), _p(gamma), _p(beta), _p(out), x2.shape[0], d, float(eps), act, _stream(x2)),
         "sbk_layernorm_f32")
    return out


def input_norm_stats(x, n_valid, per_batch, std_norm, eps, avoid_padding_norm=False):
    """x [B,T,C] normalised with the mean / std of each utterance's valid frames (per_batch False: norm_type
    "sentence") or of all valid frames of the batch ("batch"); n_valid int32 [B]."""
    lib = load()
    _dev_ok(x, n_valid)
    _f32(x)
    B, T, C = x.shape
    out = torch.empty_like(x)
    ws = torch.empty(max(1, lib.sbk_input_norm_stats_workspace_bytes(B, C) // 4), dtype=torch.float32, device=x.device)
    _chk(lib.sbk_input_norm_stats_f32(_p(x), _p(n_valid), _p(out), _p(ws), B, T, C, int(bool(per_batch)),
                                      int(bool(std_norm)), float(eps), int(bool(avoid_padding_norm)), _stream(x)),
         "sbk_input_norm_stats_f32")
    return out


def input_norm_global(x, mean, std, eps):
    lib = load()
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    _dev_ok(x2, mean, std)
    out = torch.empty_like(x)
    _chk(lib.sbk_input_norm_global_f32(_p(x2), _p(mean), _p(std), _p(out), x2.shape[0], C, float(eps), _stream(x2)),
         "sbk_input_norm_global_f32")
    return out


def input_norm_global_masked(x, mean, std, n_valid, eps):
    """``input_norm_global`` with avoid_padding_norm: x [B,T,C], the frames t >= n_valid[b] pass through unchanged."""
    lib = load()
    B, T, C = x.shape
    _dev_ok(x, mean, std, n_valid)
    _f32(x)
    out = torch.empty_like(x)
    _chk(lib.sbk_input_norm_global_masked_f32(_p(x), _p(mean), _p(std), _p(n_valid), _p(out), B, T, C, float(eps), _stream(x)),
         "sbk_input_norm_global_masked_f32")
    return out


def pcm16_to_f32(pcm: torch.Tensor, channels: int = 1, out=None):
    """int16 PCM (any shape; interleaved channels last when channels > 1) -> float32 sample / 32768, channel mean."""
    lib = load()
    _dev_ok(pcm)
    if pcm.dtype != torch.int16:
        raise SbkError(f"expected int16 PCM, got {pcm.dtype}")
    shape = pcm.shape if channels == 1 else pcm.shape[:-1]
    frames = pcm.numel() // channels
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    _chk(lib.sbk_pcm16_to_f32(_p(pcm), _p(out), frames, int(channels), _stream(pcm)), "sbk_pcm16_to_f32")
    return out


def fbank(wav, window, twiddle, radices, mel_w, mel_ptr, mel_bin, n_fft, hop, n_mels, amin, top_db,
          norm_mean=None, norm_std=None, norm_eps=1e-10):
    """[B,N] waveforms -> [B,T,n_mels] log-mel features (see include/sbk.h)."""
    lib = load()
    _dev_ok(wav, window, twiddle, mel_w, mel_ptr, mel_bin, norm_mean, norm_std)
    _f32(wav)
    B, N = wav.shape
    T = 1 + N // hop
    out = torch.empty(B, T, n_mels, dtype=torch.float32, device=wav.device)
    tile_max = torch.empty(B, (T + 3) // 4, dtype=torch.float32, device=wav.device)
    rad = (c_int32 * len(radices))(*radices)
    _chk(lib.sbk_fbank_f32(_p(wav), _p(window), _p(twiddle), rad, len(radices), _p(mel_w), _p(mel_ptr), _p(mel_bin),
                           _p(out), _p(tile_max), B, N, n_fft, hop, n_mels, mel_w.numel(), float(amin), float(top_db),
                           _p(norm_mean), _p(norm_std), float(norm_eps), _stream(wav)), "sbk_fbank_f32")
    return out


def whisper_log_mel(wav, window, twiddle, radices, mel_w, mel_ptr, mel_bin, n_fft, hop, n_mels):
    """[B,N] waveforms -> Whisper log-mel [B, n_mels, N // hop] (see include/sbk.h)."""
    lib = load()
    _dev_ok(wav, window, twiddle, mel_w, mel_ptr, mel_bin)
    _f32(wav)
    B, N = wav.shape
    T = N // hop
    tmp = torch.empty(B, T, n_mels, dtype=torch.float32, device=wav.device)
    tile_max = torch.empty(B * ((T + 3) // 4), dtype=torch.float32, device=wav.device)
    out = torch.empty(B, n_mels, T, dtype=torch.float32, device=wav.device)
    rad = (c_int32 * len(radices))(*radices)
    _chk(lib.sbk_whisper_log_mel_f32(_p(wav), _p(window), _p(twiddle), rad, len(radices), _p(mel_w), _p(mel_ptr),
                                     _p(mel_bin), _p(tmp), _p(tile_max), _p(out), B, N, n_fft, hop, n_mels,
                                     mel_w.numel(), _stream(wav)), "sbk_whisper_log_mel_f32")
    return out


def stft(wav, window, twiddle, radices, n_fft, hop):
    """[B,N] -> complex STFT [B,T,n_fft/2+1,2]."""
    lib = load()
    _dev_ok(wav, window, twiddle)
    _f32(wav)
    B, N = wav.shape
    T = 1 + N // hop
    spec = torch.empty(B, T, n_fft // 2 + 1, 2, dtype=torch.float32, device=wav.device)
    rad = (c_int32 * len(radices))(*radices)
    _chk(lib.sbk_stft_f32(_p(wav), _p(window), _p(twiddle), rad, len(radices), _p(spec), B, N, n_fft, hop, _stream(wav)),
         "sbk_stft_f32")
    return spec


def spectral_magnitude(stft_t, power=1.0, log=False, eps=1e-14):
    lib = load()
    _dev_ok(stft_t)
    _f32(stft_t)
    out = torch.empty(stft_t.shape[:-1], dtype=torch.float32, device=stft_t.device)
    _chk(lib.sbk_spectral_magnitude_f32(_p(stft_t), _p(out), out.numel(), float(power), int(bool(log)), float(eps),
                                        _stream(stft_t)), "sbk_spectral_magnitude_f32")
    return out


def amplitude_to_db(x, multiplier, amin, db_offset, top_db):
    """In place on x [B, ...]: dB conversion + per-utterance floor."""
    lib = load()
    _dev_ok(x)
    _f32(x)
    B = x.shape[0]
    tile_max = torch.empty(B, 64, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_amplitude_to_db_f32(_p(x), _p(tile_max), B, x[0].numel(), float(multiplier), float(amin),
                                     float(db_offset), float(top_db), _stream(x)), "sbk_amplitude_to_db_f32")
    return x


def conv_block(x, wt, bias, gamma, beta, cout, eps=1e-5, slope=0.01):
    """One ConvolutionFrontEnd block: x [B,T,F,Cin] -> [B,T',F',Cout] (see include/sbk.h)."""
    lib = load()
    _dev_ok(x, wt, bias, gamma, beta)
    _f32(x)
    B, Tin, Fin, Cin = x.shape
    Tout, Fout = (Tin - 1) // 2 + 1, (Fin - 1) // 2 + 1
    y = torch.empty(B, Tout, Fout, cout, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_conv_block_f32(_p(x), _p(wt), _p(bias), _p(gamma), _p(beta), _p(y), B, Tin, Fin, Cin, cout,
                                float(eps), float(slope), _stream(x)), "sbk_conv_block_f32")
    return y


def conv_block_weight(w, ksize):
    """conv.weight [Cout,Cin,kF,kT] in the layout sbk_conv_block_k_f32 reads for this shape (sbk_conv_block_k_layout): the
    tap-major rows [(ci,kf,kt), Cout] of conv_block, or the matrix-core panel [kt][kf][Cin/8][2][Cout][4]."""
    cout, cin = w.shape[0], w.shape[1]
    w = w.detach()
    if load().sbk_conv_block_k_layout(cin, cout, int(ksize)) == 1:
        return w.permute(3, 2, 1, 0).reshape(ksize, ksize, cin // 8, 2, 4, cout).permute(0, 1, 2, 3, 5, 4).contiguous()
    return w.permute(1, 2, 3, 0).reshape(-1, cout).contiguous()


def conv_block_k(x, wt, bias, gamma, beta, cout, ksize, stride, eps=1e-5, slope=0.01):
    """A ConvolutionFrontEnd block with a ksize x ksize stride-2 kernel ((3, 2) or (5, 2)): x [B,T,F,Cin] -> [B,T',F',Cout];
    ``wt`` = conv_block_weight(conv.weight, ksize) (see include/sbk.h)."""
    lib = load()
    _dev_ok(x, wt, bias, gamma, beta)
    _f32(x)
    B, Tin, Fin, Cin = x.shape
    Tout, Fout = (Tin - 1) // 2 + 1, (Fin - 1) // 2 + 1
    y = torch.empty(B, Tout, Fout, cout, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_conv_block_k_f32(_p(x), _p(wt), _p(bias), _p(gamma), _p(beta), _p(y), B, Tin, Fin, Cin, cout, int(ksize),
                                  int(stride), float(eps), float(slope), _stream(x)), "sbk_conv_block_k_f32")
    return y


def conv_block_res1x1(x, w1t, b1, gamma1, beta1, eps1, w2t, b2, gamma2, beta2, eps2, cout, slope=0.01):
    """The residual 1x1 ConvBlock in one launch: LeakyReLU(LN(conv_0(x))) + LN(reduce_conv(x)); x [B,T,F,Cin] -> [B,T,F,Cout],
    w1t / w2t [Cin,Cout]."""
    lib = load()
    _dev_ok(x, w1t, b1, gamma1, beta1, w2t, b2, gamma2, beta2)
    _f32(x)
    B, T, F, Cin = x.shape
    y = torch.empty(B, T, F, cout, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_conv_block_res1x1_f32(_p(x), _p(w1t), _p(b1), _p(gamma1), _p(beta1), float(eps1), _p(w2t), _p(b2), _p(gamma2),
                                       _p(beta2), float(eps2), _p(y), B, T, F, Cin, cout, float(slope), _stream(x)),
         "sbk_conv_block_res1x1_f32")
    return y


def relpos_attention(qkv, pos, bias_u, bias_v, key_len, H, scale, want_attn=False, chunk_size=0, left_chunks=-1,
                     out=None):
    """qkv [B,T,3*d] (per-head interleaved), pos [2T-1,d] -> context [B,T,d] (+ weights [B,H,T,T]).
    ``chunk_size`` > 0: Dynamic Chunk mask (``left_chunks`` < 0 = unlimited left context).  ``out``: optional
    contiguous [B,T,d] destination."""
    lib = load()
    _dev_ok(qkv, pos, bias_u, bias_v, key_len, out)
    _f32(qkv)
    B, T, d3 = qkv.shape
    d = d3 // 3
    if out is None:
        out = torch.empty(B, T, d, dtype=torch.float32, device=qkv.device)
    attn = torch.empty(B, H, T, T, dtype=torch.float32, device=qkv.device) if want_attn else None
    _chk(lib.sbk_relpos_attention_f32(_p(qkv), _p(pos), _p(bias_u), _p(bias_v), _p(key_len), _p(out), _p(attn), B, T,
                                      H, d // H, float(scale), int(chunk_size), int(left_chunks), _stream(qkv)),
         "sbk_relpos_attention_f32")
    return out, attn


def rope_attention(qkv, cosines, sines, key_len, H, scale, want_attn=False, chunk_size=0, left_chunks=-1, out=None,
                   out_dtype=torch.float32):
    """qkv [B,T,3*d] (per-head interleaved), cosines / sines [rows >= T, Dh] -> context [B,T,d].  ``cosines`` =
    ``sines`` = None: plain scaled-dot-product attention (no rotation; no attention-weights output)."""
    lib = load()
    _dev_ok(qkv, cosines, sines, key_len, out)
    _f32(qkv)
    B, T, d3 = qkv.shape
    d = d3 // 3
    rows = cosines.shape[0] if cosines is not None else 0
    if out_dtype == torch.bfloat16:  # bf16 operands AND a bf16 context (the operand of the output projection)
        if want_attn or d // H != 64 or out is not None:
            raise SbkError("rope_attention: the bf16 context output needs head_dim 64 and no attention-weights output")
        out = torch.empty(B, T, d, dtype=torch.bfloat16, device=qkv.device)
        _chk(lib.sbk_rope_attention_bf16o(_p(qkv), _p(cosines), _p(sines), _p(key_len), _p(out), B, T, H, d // H,
                                          rows, float(scale), int(chunk_size), int(left_chunks), _stream(qkv)),
             "sbk_rope_attention_bf16o")
        return out, None
    if out is None:
        out = torch.empty(B, T, d, dtype=torch.float32, device=qkv.device)
    if precision() == "bf16" and not want_attn and d // H == 64:  # opt-in: bf16 operands on the matrix cores
        _chk(lib.sbk_rope_attention_bf16(_p(qkv), _p(cosines), _p(sines), _p(key_len), _p(out), B, T, H, d // H,
                                         rows, float(scale), int(chunk_size), int(left_chunks), _stream(qkv)),
             "sbk_rope_attention_bf16")
        return out, None
    attn = torch.empty(B, H, T, T, dtype=torch.float32, device=qkv.device) if want_attn else None
    _chk(lib.sbk_rope_attention_f32(_p(qkv), _p(cosines), _p(sines), _p(key_len), _p(out), _p(attn), B, T, H, d // H,
                                    rows, float(scale), int(chunk_size), int(left_chunks), _stream(qkv)),
         "sbk_rope_attention_f32")
    return out, attn


def attention_bf16(qkv: torch.Tensor, key_len, H: int, scale: float):
    """Plain attention on bf16 rows: qkv [B,T,3*d] torch.bfloat16 (per-head interleaved, written by gemm_nt_bf16a) ->
    context [B,T,d] torch.bfloat16 (head_dim 64)."""
    lib = load()
    _dev_ok(qkv, key_len)
    B, T, d3 = qkv.shape
    d = d3 // 3
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous() or d // H != 64:
        raise SbkError("attention_bf16: contiguous torch.bfloat16 qkv rows with head_dim 64")
    out = torch.empty(B, T, d, dtype=torch.bfloat16, device=qkv.device)
    ws = torch.empty(lib.sbk_attention_bf16io_workspace_bytes(B, T, H) // 2, dtype=torch.bfloat16, device=qkv.device)
    _chk(lib.sbk_attention_bf16io(_p(qkv), _p(key_len), _p(out), _p(ws), B, T, H, d // H, float(scale), _stream(qkv)),
         "sbk_attention_bf16io")
    return out


def glu_dwconv(h, w, bias, ksize, chunk_size=0, out=None):
    """h [B,T,2d] -> depthwise_conv(GLU(h)) [B,T,d]; w [d,ksize]; ``chunk_size`` > 0: Dynamic Chunk Convolution."""
    lib = load()
    _dev_ok(h, w, bias, out)
    _f32(h)
    B, T, d2 = h.shape
    y = out if out is not None else torch.empty(B, T, d2 // 2, dtype=torch.float32, device=h.device)
    _chk(lib.sbk_glu_dwconv_f32(_p(h), _p(w), _p(bias), _p(y), B, T, d2 // 2, int(ksize), int(chunk_size), _stream(h)),
         "sbk_glu_dwconv_f32")
    return y


CSGU_KERNEL_SIZES = (3, 5, 7, 15, 31)  # the instantiations of csrc/csgu.hip
CSGU_GATE_ACTS = (ACT_NONE, ACT_SWISH, ACT_GELU, ACT_RELU)


def csgu(h, gamma, beta, eps, w, bias, ksize, gate_act=ACT_NONE, out=None):
    """Convolutional Spatial Gating Unit: h [B,T,2C] -> gate_act(depthwise_conv_reflect(LayerNorm(h[..., C:]))) * h[..., :C]
    [B,T,C]; gamma / beta [C], w [C,ksize], bias [C].  The reflect padding needs T > (ksize - 1) / 2."""
    lib = load()
    _dev_ok(h, gamma, beta, w, bias, out)
    _f32(h)
    B, T, C2 = h.shape
    ksize, halo = int(ksize), (int(ksize) - 1) // 2
    if ksize not in CSGU_KERNEL_SIZES:
        raise SbkError(f"csgu: kernel size {ksize} not instantiated {CSGU_KERNEL_SIZES}")
    if 0 < T <= halo:  # (F.pad(mode="reflect") refuses a padding that is not smaller than the sequence)
        raise SbkError(f"csgu: T={T} frames cannot be reflect-padded by {halo} (ksize={ksize} needs T > (ksize-1)/2)")
    y = out if out is not None else torch.empty(B, T, C2 // 2, dtype=torch.float32, device=h.device)
    stats = torch.empty(B * T * 2, dtype=torch.float32, device=h.device)
    _chk(lib.sbk_csgu_f32(_p(h), _p(gamma), _p(beta), float(eps), _p(w), _p(bias), _p(y), _p(stats), B, T, C2 // 2, ksize,
                          int(gate_act), _stream(h)), "sbk_csgu_f32")
    return y


# ------------------------------------------------------------------ wav2vec 2.0 (csrc/wav2vec2.hip)
W2V_GROUP_NORM, W2V_LAYER_NORM = 1, 2  # the ``mode`` of w2v_conv0
W2V_POSCONV_GROUP_WIDTHS = (16, 32, 48, 64)  # the instantiations of the positional convolution
W2V_CONV0_MAX_KERNEL, W2V_POSCONV_MAX_KERNEL = 16, 128


def w2v_conv0(wav, w, bias, gamma, beta, stride, mode, eps=1e-5, normalize=False, wav_eps=1e-5, out=None):
    """Layer 0 of the wav2vec 2.0 feature encoder: wav [B,N] -> GELU(norm(conv(wav))) [B,T0,C0], time-major.  w [C0,k] (the
    Conv1d weight without its unit input-channel axis), bias [C0] or None; ``mode`` W2V_GROUP_NORM (GroupNorm(C0, C0): the
    statistics of every (utterance, channel) over the T0 frames of the padded row, from a statistics launch that does not form
    the activation) or W2V_LAYER_NORM (over the channels of a frame); gamma / beta [C0].  ``normalize``: the feature
    extractor's F.layer_norm over every padded row, applied on load."""
    lib = load()
    _dev_ok(wav, w, bias, gamma, beta, out)
    _f32(wav), _f32(w)
    B, N = wav.shape
    C0, k = w.shape
    s = int(stride)
    if not (1 <= s <= k <= W2V_CONV0_MAX_KERNEL):
        raise SbkError(f"w2v_conv0: kernel {k} / stride {s} (1 <= stride <= kernel <= {W2V_CONV0_MAX_KERNEL})")
    if N < k:
        raise SbkError(f"w2v_conv0: N={N} samples are fewer than the kernel's {k}")
    if mode not in (W2V_GROUP_NORM, W2V_LAYER_NORM):
        raise SbkError(f"w2v_conv0: mode {mode}")
    T0 = (N - k) // s + 1
    y = out if out is not None else torch.empty(B, T0, C0, dtype=torch.float32, device=wav.device)
    wstat = cstat = None
    if normalize or mode == W2V_GROUP_NORM:
        wstat = torch.empty(B, 2, dtype=torch.float32, device=wav.device) if normalize else None
        cstat = torch.empty(B, C0, 2, dtype=torch.float32, device=wav.device) if mode == W2V_GROUP_NORM else None
        nbytes = lib.sbk_w2v_conv0_stats_workspace_bytes(B, N, k, s)
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=wav.device)
        _chk(lib.sbk_w2v_conv0_stats_f32(_p(wav), _p(w) if cstat is not None else None, _p(bias), int(bool(normalize)),
                                         float(wav_eps), float(eps), _p(wstat), _p(cstat), _p(ws), nbytes, B, N, C0, k, s,
                                         _stream(wav)), "sbk_w2v_conv0_stats_f32")
    _chk(lib.sbk_w2v_conv0_f32(_p(wav), _p(wstat), _p(w), _p(bias), int(mode), _p(cstat), _p(gamma), _p(beta), float(eps),
                               _p(y), B, N, C0, k, s, _stream(wav)), "sbk_w2v_conv0_f32")
    return y


def w2v_posconv(x, key_len, w, bias, groups, ksize, ln=None, out=None):
    """x [B,T,d] -> mask(x) + GELU(grouped_conv(mask(x)) + bias), the positional convolution of wav2vec 2.0 with its residual;
    ``mask`` zeroes the frames >= key_len[b] (int32 [B] or None) on read -- ``x`` is left as it is.  w [d, ksize * d/groups]:
    the effective filter tap-major (w[o, j * cg + i] = W[o, i, j]).  ``ln`` = (gamma, beta, eps): LayerNorm over d on the way
    out.  ``out`` may be a view (of anything but ``x``)."""
    lib = load()
    gamma, beta, eps = ln if ln is not None else (None, None, 0.0)
    _dev_ok(x, key_len, w, bias, gamma, beta, out)
    _f32(x), _f32(w)
    B, T, d = x.shape
    groups, ksize = int(groups), int(ksize)
    if d % groups or d // groups not in W2V_POSCONV_GROUP_WIDTHS:
        raise SbkError(f"w2v_posconv: group width {d}/{groups} not instantiated {W2V_POSCONV_GROUP_WIDTHS}")
    if not (1 <= ksize <= W2V_POSCONV_MAX_KERNEL) or tuple(w.shape) != (d, ksize * (d // groups)):
        raise SbkError(f"w2v_posconv: {ksize} taps (1..{W2V_POSCONV_MAX_KERNEL}) with a weight {tuple(w.shape)}")
    y = out if out is not None else torch.empty(B, T, d, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_w2v_posconv_f32(_p(x), _p(key_len), _p(w), _p(bias), _p(gamma), _p(beta), float(eps), _p(y), B, T, d, groups,
                                 ksize, _stream(x)), "sbk_w2v_posconv_f32")
    return y


def w2v_utt_norm(x, eps=1e-5):
    """F.layer_norm(x, x.shape[-2:]) without affine: every [T', d] block of x [..., T', d] over all of its values."""
    lib = load()
    _dev_ok(x)
    _f32(x)
    n = x.shape[-2] * x.shape[-1]
    y = torch.empty_like(x)
    _chk(lib.sbk_w2v_utt_norm_f32(_p(x), _p(y), x.numel() // n if n else 0, n, float(eps), _stream(x)), "sbk_w2v_utt_norm_f32")
    return y


# ------------------------------------------------------------------ WavLM (csrc/wavlm.hip)
WAVLM_HEAD_DIMS = (16, 32, 64)  # the instantiations of the gated relative-position attention


def wavlm_attention(qkv, x, gate_w, gate_b, gate_const, tab, key_len, H, scale, out=None):
    """WavLM's self-attention: qkv [B,T,3*d] (per-head interleaved), x [B,T,d] the hidden states the attention module received,
    gate_w [8,Dh] / gate_b [8] (gru_rel_pos_linear), gate_const [H] (gru_rel_pos_const, any shape of H values), tab [H,2T-1]
    (``wavlm_bias_table``) -> context [B,T,d].  score = scale * q.k + gate(x)[b,h,i] * tab[h, j - i + T - 1] over the keys
    j < key_len[b]; no [T,T] tensor is formed."""
    lib = load()
    _dev_ok(qkv, x, gate_w, gate_b, gate_const, tab, key_len, out)
    _f32(qkv), _f32(x), _f32(gate_w), _f32(tab)
    B, T, d3 = qkv.shape
    d = d3 // 3
    Dh = d // H
    if Dh not in WAVLM_HEAD_DIMS:
        raise NotImplementedError(f"wavlm_attention: head dim {d}/{H} not instantiated {WAVLM_HEAD_DIMS}")
    max_t = lib.sbk_wavlm_attention_max_frames()
    if T > max_t:
        raise SbkError(f"wavlm_attention: T={T} frames exceed the {max_t} whose bias table row fits the kernel's 64 KiB of LDS")
    if tuple(x.shape) != (B, T, d) or tuple(gate_w.shape) != (8, Dh) or gate_b.numel() != 8 or gate_const.numel() != H \
            or (T and tuple(tab.shape) != (H, 2 * T - 1)):
        raise SbkError(f"wavlm_attention: x {tuple(x.shape)}, gate_w {tuple(gate_w.shape)}, gate_b {tuple(gate_b.shape)}, "
                       f"gate_const {tuple(gate_const.shape)}, tab {tuple(tab.shape)} for B={B} T={T} H={H} Dh={Dh}")
    _f32(gate_b), _f32(gate_const)
    if out is None:
        out = torch.empty(B, T, d, dtype=torch.float32, device=qkv.device)
    _chk(lib.sbk_wavlm_attention_f32(_p(qkv), _p(x), _p(gate_w), _p(gate_b), _p(gate_const), _p(tab), _p(key_len), _p(out),
                                     B, T, H, Dh, float(scale), _stream(qkv)), "sbk_wavlm_attention_f32")
    return out


# ------------------------------------------------------------------ HyperMixing (csrc/hypermix.hip)
HYPERMIX_MAX_HEAD_DIM, HYPERMIX_MAX_HYPER_PER_HEAD, HYPERMIX_MAX_FRAMES, HYPERMIX_MAX_WIDTH = 64, 256, 3000, 1024
HYPERMIX_SPLIT_FRAMES = 256  # csrc/hypermix.hip kSplitFrames (sbk_hypermix_split_frames; tests check the two agree)
_GEN_KEYS = ("fc1_weights", "fc1_biases", "fc2_weights", "fc2_biases")


def hypermix_split_frames() -> int:
    """Frames of one piece of the time reduction: ``hypermix`` sums T frames in ceil(T / this) pieces, combined in order."""
    return int(load().sbk_hypermix_split_frames())


def hypermix(h, key_len, pe, w1_gen, w2_gen, ln_w, ln_b, eps, H, residual=None, out=None):
    """HyperMixing token mixing + LayerNorm (+ skip) in two launches (three when T exceeds ``hypermix_split_frames()``).
    h [B,T,d] the normed input; key_len int32 [B] or None; pe [>=T,d] the mixer's position table (its first T rows are read);
    w1_gen / w2_gen the two generators as (fc1_weights [H,Dh,Dh], fc1_biases [H,Dh], fc2_weights [H,k,Dh], fc2_biases [H,k]) or a
    mapping with those keys; ln_w, ln_b [d].  Returns LayerNorm(mix(h)) + residual, [B,T,d]; rows past key_len[b] are ln_b +
    residual and never read h.  ``out`` may be ``residual`` itself, never ``h``.  The generated [B,H,T,k] weights are not formed;
    the intermediates ([B,H,Dh,Dh+1] matrices) live in the current stream's grow-only workspace."""
    lib = load()
    gens = [tuple(g[k] for k in _GEN_KEYS) if hasattr(g, "keys") else tuple(g) for g in (w1_gen, w2_gen)]
    flat = [t for g in gens for t in g]
    _dev_ok(h, key_len, pe, ln_w, ln_b, residual, out, *flat)
    for t in (h, pe, ln_w, ln_b, residual, out, *flat):
        if t is not None:
            _f32(t)
    if h.dim() != 3:
        raise SbkError(f"hypermix: h {tuple(h.shape)} is not [B,T,d]")
    B, T, d = h.shape
    H = int(H)
    if H <= 0 or d % H:
        raise SbkError(f"hypermix: d={d} is not divisible by num_heads={H} (d % H == 0 is required)")
    Dh = d // H
    k = gens[0][2].shape[1] if gens[0][2].dim() == 3 else -1
    if Dh > HYPERMIX_MAX_HEAD_DIM:
        raise SbkError(f"hypermix: head width Dh={Dh} exceeds the limit Dh <= {HYPERMIX_MAX_HEAD_DIM}")
    if k > HYPERMIX_MAX_HYPER_PER_HEAD:
        raise SbkError(f"hypermix: hypernet width per head k={k} exceeds the limit k <= {HYPERMIX_MAX_HYPER_PER_HEAD}")
    if T > HYPERMIX_MAX_FRAMES:
        raise SbkError(f"hypermix: T={T} frames exceed the limit T <= {HYPERMIX_MAX_FRAMES}")
    if d > HYPERMIX_MAX_WIDTH:
        raise SbkError(f"hypermix: d={d} exceeds the limit d <= {HYPERMIX_MAX_WIDTH}")
    want = ((H, Dh, Dh), (H, Dh), (H, k, Dh), (H, k))
    for name, g in zip(("w1_gen", "w2_gen"), gens):
        if len(g) != 4 or any(tuple(t.shape) != w for t, w in zip(g, want)):
            raise SbkError(f"hypermix: {name} {[tuple(t.shape) for t in g]} is not {want} for d={d} H={H}")
    if pe.dim() != 2 or pe.shape[1] != d or pe.shape[0] < T or ln_w.numel() != d or ln_b.numel() != d:
        raise SbkError(f"hypermix: pe {tuple(pe.shape)}, ln_w {tuple(ln_w.shape)}, ln_b {tuple(ln_b.shape)} for T={T} d={d}")
    if key_len is not None and (key_len.dtype != torch.int32 or key_len.numel() != B):
        raise SbkError(f"hypermix: key_len must be int32 [{B}]")
    if residual is not None and tuple(residual.shape) != (B, T, d):
        raise SbkError(f"hypermix: residual {tuple(residual.shape)} for h {tuple(h.shape)}")
    if out is None:
        out = torch.empty(B, T, d, dtype=torch.float32, device=h.device)
    elif tuple(out.shape) != (B, T, d):
        raise SbkError(f"hypermix: out {tuple(out.shape)} for h {tuple(h.shape)}")
    if B * T and out.data_ptr() == h.data_ptr():
        raise SbkError("hypermix: out must not alias h (it may alias residual)")
    if B == 0 or T == 0:
        return out
    nbytes = lib.sbk_hypermix_workspace_bytes(B, T, H, Dh)
    st = _stream(h)
    with _Workspace(nbytes, h.device, per_stream=True) as ws:
        _chk(lib.sbk_hypermix_f32(_p(h), _p(key_len), _p(pe), *[_p(t) for t in flat], _p(ln_w), _p(ln_b), float(eps),
                                  _p(residual), _p(out), ws.ptr, nbytes, B, T, H, Dh, k, st), "sbk_hypermix_f32")
    return out


# ------------------------------------------------------------------ recurrent layers (csrc/rnn.hip)
RNN_LSTM = 0  # SBK_RNN_LSTM
RNN_MAX_HIDDEN = 2048  # csrc/rnn.hip kMaxH


def rnn_layer_route(B, T, H, D) -> int:
    """The route ``rnn_layer(route=0)`` takes for a shape: 1 = step launches; 0 = the shape is refused."""
    return int(load().sbk_rnn_layer_route(int(B), int(T), int(H), int(D)))


def rnn_layer(xp, w_hh, b_ih=None, b_hh=None, h0=None, c0=None, route=0):
    """One LSTM layer for every utterance and direction (sbk_rnn_layer_f32): xp [B,T,D,4H] = x . W_ih^T per direction without
    bias, w_hh [D,4H,H], b_ih / b_hh [D,4H] or None, h0 / c0 [D,B,H] or None (zeros)
    -> (out [B,T,D*H], hn [D,B,H], cn [D,B,H]); direction 1 runs backwards in time and writes at its own t."""
    lib = load()
    if xp.ndim != 4 or w_hh.ndim != 3:
        raise SbkError(f"rnn_layer: xp {tuple(xp.shape)} is not [B,T,D,4H] or w_hh {tuple(w_hh.shape)} is not [D,4H,H]")
    B, T, D, G = xp.shape
    H = w_hh.shape[2]
    if G != 4 * H or tuple(w_hh.shape) != (D, 4 * H, H):
        raise SbkError(f"rnn_layer: xp {tuple(xp.shape)} and w_hh {tuple(w_hh.shape)} do not agree on D and H")
    for name, t, want in (("b_ih", b_ih, (D, 4 * H)), ("b_hh", b_hh, (D, 4 * H)), ("h0", h0, (D, B, H)), ("c0", c0, (D, B, H))):
        if t is not None and tuple(t.shape) != want:
            raise SbkError(f"rnn_layer: {name} {tuple(t.shape)} is not {want}")
    _dev_ok(xp, w_hh, b_ih, b_hh, h0, c0)
    for t in (xp, w_hh, b_ih, b_hh, h0, c0):
        if t is not None:
            _f32(t)
    out = torch.empty(B, T, D * H, dtype=torch.float32, device=xp.device)
    hn = torch.empty(D, B, H, dtype=torch.float32, device=xp.device)
    cn = torch.empty(D, B, H, dtype=torch.float32, device=xp.device)
    _chk(lib.sbk_rnn_layer_f32(_p(xp), _p(w_hh), _p(b_ih), _p(b_hh), _p(h0), _p(c0), _p(out), _p(hn), _p(cn), B, T, H, D,
                               RNN_LSTM, int(route), _stream(xp)), "sbk_rnn_layer_f32")
    return out, hn, cn


# ------------------------------------------------------------------ GRU attention decoder (csrc/attn_rnn.hip)
def attn_rnn_attend(enc, enc_h, enc_len, dec_h, attn_v, prev_attn=None, conv_w=None, loc_w=None, loc_b=None, scaling=1.0,
                    row_utt=None):
    """One attention step for n rows (sbk_attn_rnn_attend_f32): enc [B,T,E], enc_h [B,T,A], enc_len [B] int32, dec_h [n,A],
    attn_v [A]; location-aware with prev_attn [n,T], conv_w [C,2k+1], loc_w [A,C], loc_b [A], content-based without them;
    row_utt [n] int32 or None (identity, n == B) -> (attn [n,T], ctx [n,E])."""
    lib = load()
    B, T, E = enc.shape
    n, A = dec_h.shape
    C, k = (conv_w.shape[0], (conv_w.shape[-1] - 1) // 2) if conv_w is not None else (0, 0)
    want = [("enc_h", enc_h, (B, T, A)), ("enc_len", enc_len, (B,)), ("attn_v", attn_v, (A,))]
    if C:
        conv_w = conv_w.reshape(C, 2 * k + 1)
        want += [("prev_attn", prev_attn, (n, T)), ("loc_w", loc_w, (A, C)), ("loc_b", loc_b, (A,))]
    if row_utt is not None:
        want.append(("row_utt", row_utt, (n,)))
    for name, t, shape in want:
        if t is None or tuple(t.shape) != shape:
            raise SbkError(f"attn_rnn_attend: {name} {None if t is None else tuple(t.shape)} is not {shape}")
    _dev_ok(enc, enc_h, enc_len, dec_h, attn_v, prev_attn, conv_w, loc_w, loc_b, row_utt)
    for t in (enc, enc_h, dec_h, attn_v, prev_attn, conv_w, loc_w, loc_b):
        if t is not None:
            _f32(t)
    for t in (enc_len, row_utt):
        if t is not None and t.dtype != torch.int32:
            raise SbkError(f"attn_rnn_attend: expected int32 lengths / rows, got {t.dtype}")
    attn = torch.empty(n, T, dtype=torch.float32, device=enc.device)
    ctx = torch.empty(n, E, dtype=torch.float32, device=enc.device)
    nbytes = lib.sbk_attn_rnn_attend_workspace_bytes(n, T)
    ws = _Workspace(nbytes, enc.device)
    _chk(lib.sbk_attn_rnn_attend_f32(_p(enc), _p(enc_h), _p(enc_len), _p(row_utt), _p(dec_h), _p(prev_attn), _p(conv_w), _p(loc_w),
                                     _p(loc_b), _p(attn_v), float(scaling), _p(attn), _p(ctx), ws.ptr, nbytes, n, B, T, A, E, C, k,
                                     _stream(enc)), "sbk_attn_rnn_attend_f32")
    return attn, ctx


def attn_rnn_attn_init(enc_len, T, row_utt=None):
    """The first prev_attn (sbk_attn_rnn_attn_init_f32): 1 / enc_len[u] on the valid frames of each row, 0 behind -> [n,T]."""
    lib = load()
    _dev_ok(enc_len, row_utt)
    B = enc_len.shape[0]
    n = row_utt.shape[0] if row_utt is not None else B
    attn = torch.empty(n, int(T), dtype=torch.float32, device=enc_len.device)
    _chk(lib.sbk_attn_rnn_attn_init_f32(_p(enc_len), _p(row_utt), _p(attn), n, B, int(T), _stream(attn)),
         "sbk_attn_rnn_attn_init_f32")
    return attn


def gru_cell(gi, gh, b_ih=None, b_hh=None, h_prev=None, out=None):
    """torch.nn.GRUCell's update (sbk_gru_cell_f32): gi, gh [n,3H] without bias, b_ih / b_hh [3H] (both or neither), h_prev [n,H]
    or None (zeros) -> h' [n,H]; ``out`` may be ``h_prev``."""
    lib = load()
    n, G = gi.shape
    H = G // 3
    if G != 3 * H or tuple(gh.shape) != (n, G):
        raise SbkError(f"gru_cell: gi {tuple(gi.shape)} and gh {tuple(gh.shape)} are not both [n,3H]")
    for name, t, shape in (("b_ih", b_ih, (G,)), ("b_hh", b_hh, (G,)), ("h_prev", h_prev, (n, H)), ("out", out, (n, H))):
        if t is not None and tuple(t.shape) != shape:
            raise SbkError(f"gru_cell: {name} {tuple(t.shape)} is not {shape}")
    _dev_ok(gi, gh, b_ih, b_hh, h_prev, out)
    for t in (gi, gh, b_ih, b_hh, h_prev, out):
        if t is not None:
            _f32(t)
    if out is None:
        out = torch.empty(n, H, dtype=torch.float32, device=gi.device)
    _chk(lib.sbk_gru_cell_f32(_p(gi), _p(gh), _p(b_ih), _p(b_hh), _p(h_prev), _p(out), n, H, _stream(gi)), "sbk_gru_cell_f32")
    return out


class AttnRNNPrepared:
    """An AttentionalRNNDecoder (GRU cells, location-aware or content-based attention), and for the search its embedding and
    output layer, in the layouts of sbk_attn_rnn_weights (include/sbk.h).  The tensors are kept alive here for as long as the
    struct points at them."""

    def __init__(self, gru_layers, attn, proj_w, proj_b, scaling, emb=None, fc_w=None, fc_b=None):
        """gru_layers: [(w_ih, w_hh, b_ih or None, b_hh or None)] * L; attn: a dict with enc_w, enc_b, dec_w, dec_b, attn_v,
        out_w, out_b and -- location-aware -- conv_w [C,2k+1], loc_w, loc_b (all fp32 on one device)."""
        if not 1 <= len(gru_layers) <= ATTN_RNN_MAX_LAYERS:
            raise SbkError(f"AttentionalRNNDecoder: {len(gru_layers)} GRU layers (1..{ATTN_RNN_MAX_LAYERS} supported)")
        self.W, self._keep = W, keep = AttnRNNWeights(), []
        ptr = _keeper(keep, strict=False)
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(gru_layers):
            W.w_ih[l], W.w_hh[l], W.b_ih[l], W.b_hh[l] = ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh)
        for name in ("enc_w", "enc_b", "dec_w", "dec_b", "attn_v", "conv_w", "loc_w", "loc_b", "out_w", "out_b"):
            setattr(W, name, ptr(attn.get(name)))
        W.proj_w, W.proj_b, W.emb, W.fc_w, W.fc_b = ptr(proj_w), ptr(proj_b), ptr(emb), ptr(fc_w), ptr(fc_b)
        conv_w = attn.get("conv_w")
        W.n_layers, W.hidden = len(gru_layers), gru_layers[0][1].shape[1]
        W.attn_dim, W.enc_dim = attn["enc_w"].shape
        W.in_dim = gru_layers[0][0].shape[1] - W.attn_dim
        if tuple(attn["out_w"].shape) != (W.attn_dim, W.enc_dim) or tuple(proj_w.shape) != (W.hidden, W.attn_dim + W.hidden):
            raise SbkError("AttentionalRNNDecoder: the context's width (mlp_out) must equal attn_dim, and proj takes [c || cell_out]")
        W.channels, W.kernel = (conv_w.shape[0], (conv_w.shape[-1] - 1) // 2) if conv_w is not None else (0, 0)
        W.vocab, W.n_emb = (fc_w.shape[0] if fc_w is not None else 0), (emb.shape[0] if emb is not None else 0)
        if emb is not None and emb.shape[1] != W.in_dim:
            raise SbkError(f"S2SRNNGreedySearcher: embedding width {emb.shape[1]} is not the decoder's input size {W.in_dim}")
        W.scaling = float(scaling)
        self.device = keep[0].device


def attn_rnn_greedy(prep: AttnRNNPrepared, enc, enc_len, max_steps, bos, eos, check_every=8):
    """sbk_attn_rnn_greedy_f32: enc [B,T,E], enc_len [B] int32 -> (tokens [B,max_steps] int32 (eos-latched), scores
    [B,max_steps], steps_run)."""
    lib = load()
    _dev_ok(enc, enc_len)
    _f32(enc)
    B, T, _ = enc.shape
    L = int(max_steps)
    out_tok = torch.empty(B, L, dtype=torch.int32, device=enc.device)
    out_sc = torch.empty(B, L, dtype=torch.float32, device=enc.device)
    nbytes = lib.sbk_attn_rnn_greedy_workspace_bytes(ctypes.byref(prep.W), B, T)
    ws = _Workspace(nbytes, enc.device)
    steps = c_int32(0)
    _chk(lib.sbk_attn_rnn_greedy_f32(ctypes.byref(prep.W), _p(enc), _p(enc_len), ws.ptr, nbytes, _p(out_tok), _p(out_sc),
                                     ctypes.byref(steps), B, T, L, int(bos), int(eos), int(check_every), _stream(enc)),
         "sbk_attn_rnn_greedy_f32")
    return out_tok, out_sc, steps.value


def attn_rnn_decode(prep: AttnRNNPrepared, inp, enc, enc_len):
    """sbk_attn_rnn_decode_f32 (teacher forced): inp [B,L,in], enc [B,T,E], enc_len [B] int32 -> (outputs [B,L,H],
    attn [B,L,T], hs [n_layers,B,H], c [B,A])."""
    lib = load()
    _dev_ok(inp, enc, enc_len)
    _f32(inp), _f32(enc)
    B, T, _ = enc.shape
    L, W = inp.shape[1], prep.W
    if inp.shape[0] != B or inp.shape[2] != W.in_dim:
        raise SbkError(f"attn_rnn_decode: inp {tuple(inp.shape)} is not [{B},L,{W.in_dim}]")
    dev = enc.device
    outputs = torch.empty(B, L, W.hidden, dtype=torch.float32, device=dev)
    attn = torch.empty(B, L, T, dtype=torch.float32, device=dev)
    hs = torch.empty(W.n_layers, B, W.hidden, dtype=torch.float32, device=dev)
    c = torch.empty(B, W.attn_dim, dtype=torch.float32, device=dev)
    nbytes = lib.sbk_attn_rnn_decode_workspace_bytes(ctypes.byref(W), B, T)
    ws = _Workspace(nbytes, dev)
    _chk(lib.sbk_attn_rnn_decode_f32(ctypes.byref(W), _p(inp), _p(enc), _p(enc_len), ws.ptr, nbytes, _p(outputs), _p(attn), _p(hs),
                                     _p(c), B, T, L, _stream(enc)), "sbk_attn_rnn_decode_f32")
    return outputs, attn, hs, c


# ------------------------------------------------------------------ CRDNN convolution blocks (csrc/crdnn.hip)
CRDNN_MAX_FRAME = 16384  # csrc/crdnn.hip kMaxFrame: F * C floats of a frame held in LDS
CRDNN_COL_BYTES = 256 << 20  # budget of the patch matrix of one chunk of frames


def _crdnn_time_check(T, F):
    if T < 2 or F < 2:  # (F.pad(mode="reflect") of the reference refuses a padding that is not smaller than the dimension)
        raise ValueError(f"CRDNN convolution: reflect padding of 1 needs at least 2 frames and 2 bins, got T={T} F={F}")


def crdnn_conv1(x, w9, bias, gamma, beta, eps=1e-5, slope=0.01):
    """reflect-pad(1) + Conv2d(3x3) of ONE input channel + LayerNorm over (F,C) + LeakyReLU (sbk_crdnn_conv1_f32):
    x [B,T,F], w9 [9,C] (row kf*3+kt), bias [C], gamma / beta [F*C] -> [B,T,F,C]."""
    lib = load()
    B, T, F = x.shape
    C = w9.shape[1]
    _crdnn_time_check(T, F)
    _dev_ok(x, w9, bias, gamma, beta)
    y = torch.empty(B, T, F, C, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_crdnn_conv1_f32(_p(_f32(x)), _p(w9), _p(bias), _p(gamma), _p(beta), _p(y), B, T, F, C, float(eps),
                                 float(slope), _stream(x)), "sbk_crdnn_conv1_f32")
    return y


def crdnn_conv(x, wk, bias, col_bytes=None):
    """reflect-pad(1) + Conv2d(3x3, stride 1, bias) as a contraction on the matrix cores: x [B,T,F,Cin], wk [Cout, 9*Cin] =
    conv.weight permuted to (Cout, kF, kT, Cin) -> [B,T,F,Cout].  The patch matrix (sbk_crdnn_im2col_f32) is formed for a run
    of frames that fits ``col_bytes`` (CRDNN_COL_BYTES) at a time and contracted by ``gemm_nt``'s routing."""
    lib = load()
    B, T, F, Cin = x.shape
    Cout, K = wk.shape
    if K != 9 * Cin:
        raise SbkError(f"crdnn_conv: weight {tuple(wk.shape)} for {Cin} input channels (expected [Cout, {9 * Cin}])")
    _crdnn_time_check(T, F)
    _dev_ok(x, wk, bias)
    _f32(x)
    y = torch.empty(B, T, F, Cout, dtype=torch.float32, device=x.device)
    y2 = y.view(B * T * F, Cout)
    per = min(B * T, max(1, int(col_bytes or CRDNN_COL_BYTES) // (F * K * 4)))
    st = _stream(x)
    # the patch matrix lives in the current stream's grow-only buffer: one bounded allocation per stream, reused by every chunk,
    # every convolution and every later batch (stream order makes the reuse safe)
    with _Workspace(per * F * K * 4, x.device, per_stream=True) as ws:
        for f0 in range(0, B * T, per):
            n = min(per, B * T - f0)
            col = ws.buf[ws.off:ws.off + n * F * K * 4].view(torch.float32).view(n * F, K)
            _chk(lib.sbk_crdnn_im2col_f32(_p(x), _p(col), B, T, F, Cin, f0, n, st), "sbk_crdnn_im2col_f32")
            with precision_scope("fp32"):
                gemm_nt(col, wk, bias, out=y2[f0 * F:(f0 + n) * F])
    return y


def crdnn_norm_pool(x, gamma, beta, pool_f=1, pool_t=1, eps=1e-5, slope=0.01):
    """max-pool over pool_t frames and pool_f bins of LeakyReLU(LayerNorm over (F,C)) in one pass (sbk_crdnn_norm_pool_f32):
    x [B,T,F,C] -> [B,T//pool_t,F//pool_f,C]."""
    lib = load()
    B, T, F, C = x.shape
    if T // pool_t < 1 or F // pool_f < 1:
        raise ValueError(f"CRDNN pooling: T={T} F={F} pooled by ({pool_t}, {pool_f}) leaves an empty output")
    _dev_ok(x, gamma, beta)
    y = torch.empty(B, T // pool_t, F // pool_f, C, dtype=torch.float32, device=x.device)
    _chk(lib.sbk_crdnn_norm_pool_f32(_p(_f32(x)), _p(gamma), _p(beta), _p(y), B, T, F, C, int(pool_f), int(pool_t), float(eps),
                                     float(slope), _stream(x)), "sbk_crdnn_norm_pool_f32")
    return y


def wavlm_relative_buckets(rel, num_buckets, max_distance):
    """transformers' WavLMAttention._relative_positions_bucket on an int64 CPU tensor of relative positions (key - query): half
    the buckets per sign, exact below num_buckets/4, logarithmic up to max_distance, then saturated.  float32 on the host, the
    reference's operation order: the bucket edges do not depend on a device's ``log``."""
    nb = num_buckets // 2
    buckets = (rel > 0).to(torch.long) * nb
    rel = torch.abs(rel)
    max_exact = nb // 2
    large = torch.log(rel.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(rel < max_exact, rel, large)


def wavlm_bias_table(rel_attn_embed_weight, T, num_buckets, max_distance, derived=None):
    """rel_attn_embed.weight [num_buckets, H] -> tab [H, 2T-1] on the weight's device: tab[h, r + T - 1] =
    weight[bucket(r), h] for r = key - query in [-(T-1), T-1] (= compute_bias(T, T)[h, i, i + r]).  ``derived``: a
    ``Derived`` to cache it in, keyed on the parameter and (T, num_buckets, max_distance)."""
    w = rel_attn_embed_weight

    def build():
        idx = wavlm_relative_buckets(torch.arange(-(T - 1), T, dtype=torch.long), num_buckets, max_distance)
        return w.detach().float().t().contiguous()[:, idx.to(w.device)].contiguous()

    if derived is None:
        with torch.no_grad():
            return build()
    return derived.get((w,), build, extra=(int(T), int(num_buckets), int(max_distance)))


# ------------------------------------------------------------------ decoder / searchers
def _keeper(keep, strict):
    """``ptr(t)`` for filling a weights struct: the address of ``t``, detached and contiguous and appended to ``keep`` so that
    it stays valid.  ``strict`` (the handles): anything but an fp32 device tensor raises; otherwise (the transducer / RNNLM
    layouts) the tensor is converted with ``.float()`` and None gives NULL."""
    def ptr(t):
        if t is None and not strict:
            return None
        t = t.detach().contiguous() if strict else t.detach().float().contiguous()
        if strict:
            _dev_ok(t)
            _f32(t)
        keep.append(t)
        return t.data_ptr()

    return ptr


class DecoderHandle:
    """Device pointers of a TransformerASR decoder (+ seq_lin) laid out as sbk_decoder_weights.
    Holds references to the parameter tensors so the pointers stay valid."""

    def __init__(self, model, seq_lin=None, fold=True):
        dec = model.decoder
        layers = []
        for L in dec.layers:
            if not L.normalize_before:
                raise NotImplementedError("post-norm decoder layers are not on the Conformer ASR path")
            layers.append(dict(
                ln1=(L.norm1.norm.weight, L.norm1.norm.bias), sa_in=(L.self_attn.att.in_proj_weight, L.self_attn.att.in_proj_bias),
                sa_out=(L.self_attn.att.out_proj.weight, L.self_attn.att.out_proj.bias),
                ln2=(L.norm2.norm.weight, L.norm2.norm.bias),
                ca_in=(L.multihead_attn.att.in_proj_weight, L.multihead_attn.att.in_proj_bias),
                ca_out=(L.multihead_attn.att.out_proj.weight, L.multihead_attn.att.out_proj.bias),
                ln3=(L.norm3.norm.weight, L.norm3.norm.bias), ff1=(L.pos_ffn.ffn[0].weight, L.pos_ffn.ffn[0].bias),
                ff2=(L.pos_ffn.ffn[3].weight, L.pos_ffn.ffn[3].bias)))
        pe = self._decoder_pe(model)
        self._build(layers, emb=model.custom_tgt_module.layers[0].emb.Embedding.weight,
                    pe=pe.reshape(pe.shape[-2], pe.shape[-1]), final_ln=(dec.norm.norm.weight, dec.norm.norm.bias),
                    seq=(seq_lin.w.weight, seq_lin.w.bias) if seq_lin is not None else None, nhead=dec.layers[0].nhead,
                    ffn_act=dec.layers[-1].pos_ffn.act_code, ln_eps=dec.norm.eps, emb_scale=0.0, fold=fold)
        self.key = self.source_key(model, seq_lin)

    @staticmethod
    def _decoder_pe(model):
        """The absolute table the target positions come from: positional_encoding_decoder where the encoder's attention type
        replaced positional_encoding (RelPosMHAXL, RoPEMHA), else positional_encoding itself (regularMHA; TransformerASR.py:449-457)."""
        holder = getattr(model, "positional_encoding_decoder", None)
        return (holder if holder is not None else model.positional_encoding).pe

    @classmethod
    def from_tensors(cls, layers, emb, pe, final_ln, seq, nhead, ffn_act, ln_eps, emb_scale, fold=True, key=None):
        """A pre-norm Transformer decoder given as plain tensors: ``layers`` = dicts with ln1 / sa_in / sa_out / ln2 /
        ca_in / ca_out / ln3 / ff1 / ff2 -> (weight, bias) (in_proj stacked [3d,d] as torch.nn.MultiheadAttention);
        ``emb_scale`` multiplies the token embedding (0 = sqrt(d_model)); ``seq`` = output projection (weight, bias)."""
        self = cls.__new__(cls)
        self._build(layers, emb, pe, final_ln, seq, nhead, ffn_act, ln_eps, emb_scale, fold)
        self.key = key
        return self

    def _build(self, layer_specs, emb, pe, final_ln, seq, nhead, ffn_act, ln_eps, emb_scale, fold):
        self.keep = []
        fold = fold and final_ln[0].shape[0] in (128, 256, 512)  # shapes the fused kernel takes
        layers = (DecoderLayer * len(layer_specs))()
        ptr = _keeper(self.keep, strict=True)
        dm = emb.shape[1]

        def image(kind, w):  # the handle's own image of w where the kernels that read it take the shape, else NULL: "x3" for the
            # big contractions of the search (bf16 matrix pipe), "x3p" for the decode step's projections (sbk_gemm_nt_x3r)
            N, K = w.shape
            if not (F32X3 and (_x3_shape(N, K) if kind == "x3" else X3R and K % 256 == 0 and N % 4 == 0)):
                return None
            self.keep.append(_make_image(w, kind)[0])
            return self.keep[-1].data_ptr()

        for l, S in enumerate(layer_specs):
            o = layers[l]
            o.ln1_g, o.ln1_b = map(ptr, S["ln1"])
            o.sa_in_w, o.sa_in_b = map(ptr, S["sa_in"])
            o.sa_out_w, o.sa_out_b = map(ptr, S["sa_out"])
            o.ln2_g, o.ln2_b = map(ptr, S["ln2"])
            o.ca_in_w, o.ca_in_b = map(ptr, S["ca_in"])
            o.ca_out_w, o.ca_out_b = map(ptr, S["ca_out"])
            o.ln3_g, o.ln3_b = map(ptr, S["ln3"])
            o.ff1_w, o.ff1_b = map(ptr, S["ff1"])
            o.ff2_w, o.ff2_b = map(ptr, S["ff2"])
            o.ca_kv_w3 = image("x3", S["ca_in"][0][dm:])
            o.sa_in_wp, o.sa_out_wp = image("x3p", S["sa_in"][0]), image("x3p", S["sa_out"][0])
            o.ca_q_wp, o.ca_out_wp = image("x3p", S["ca_in"][0][:dm]), image("x3p", S["ca_out"][0])
            o.ff1_wp, o.ff2_wp = image("x3p", S["ff1"][0]), image("x3p", S["ff2"][0])
            if fold:  # LayerNorm folded into the projection it feeds (fused kernels, csrc/gemm.hip)
                for name, (wf, bf) in (("sa_in", _fold_ln(*S["sa_in"], *S["ln1"])),
                                       ("ca_q", _fold_ln(S["ca_in"][0][:dm], S["ca_in"][1][:dm], *S["ln2"])),
                                       ("ff1", _fold_ln(*S["ff1"], *S["ln3"]))):
                    setattr(o, name + "_wf", ptr(wf))
                    setattr(o, name + "_bf", ptr(bf))
                    setattr(o, name + "_wfp", image("x3p", wf))  # (ABI 9: the same fold for the rows sbk_gemm_ln_nt_x3r takes)
        self.layers = layers
        W = DecoderWeights()
        W.layers = ctypes.cast(layers, POINTER(DecoderLayer))
        W.emb, W.pe = ptr(emb), ptr(pe)
        W.final_ln_g, W.final_ln_b = map(ptr, final_ln)
        if seq is not None:
            W.seq_w, W.seq_b = map(ptr, seq)
            W.seq_w3, W.seq_wp = image("x3", seq[0]), image("x3p", seq[0])
            if fold:
                wf, bf = _fold_ln(seq[0], seq[1], *final_ln)
                W.seq_wf, W.seq_bf, W.seq_wfp = ptr(wf), ptr(bf), image("x3p", wf)
        W.d_model, W.nhead = dm, nhead
        W.d_ffn, W.n_layers = layer_specs[0]["ff1"][0].shape[0], len(layer_specs)
        W.vocab = seq[0].shape[0] if seq is not None else emb.shape[0]
        W.max_len, W.ffn_act, W.ln_eps, W.emb_scale = pe.shape[-2], ffn_act, ln_eps, float(emb_scale)
        self.W, self.device = W, emb.device
        self.ready = _Ready(emb.device)  # (the folded / split tables above were written on this thread's stream)

    @staticmethod
    def source_key(model, seq_lin=None):
        """``source_key`` of every tensor the handle was derived from (the folded LayerNorm copies go stale with them)."""
        src = list(model.decoder.parameters())
        src.append(model.custom_tgt_module.layers[0].emb.Embedding.weight)
        src.append(DecoderHandle._decoder_pe(model))
        if seq_lin is not None:
            src.extend(seq_lin.parameters())
        return source_key(src)

    def stale(self, model, seq_lin=None):
        return self.source_key(model, seq_lin) != self.key


class LMHandle:
    """Device pointers of a TransformerLM laid out as sbk_lm_weights (keeps the tensors alive)."""

    def __init__(self, lm):
        self.keep = []
        ptr = _keeper(self.keep, strict=True)
        enc = lm.encoder
        layers = (LMLayer * len(enc.layers))()
        for l, L in enumerate(enc.layers):
            o = layers[l]
            o.in_w, o.in_b = ptr(L.self_att.att.in_proj_weight), ptr(L.self_att.att.in_proj_bias)
            o.out_w, o.out_b = ptr(L.self_att.att.out_proj.weight), ptr(L.self_att.att.out_proj.bias)
            o.ln1_g, o.ln1_b = ptr(L.norm1.norm.weight), ptr(L.norm1.norm.bias)
            o.ff1_w, o.ff1_b = ptr(L.pos_ffn.ffn[0].weight), ptr(L.pos_ffn.ffn[0].bias)
            o.ff2_w, o.ff2_b = ptr(L.pos_ffn.ffn[3].weight), ptr(L.pos_ffn.ffn[3].bias)
            o.ln2_g, o.ln2_b = ptr(L.norm2.norm.weight), ptr(L.norm2.norm.bias)
        self.layers = layers
        W = LMWeights()
        W.layers = ctypes.cast(layers, POINTER(LMLayer))
        emb = lm.custom_src_module.emb.Embedding.weight
        pe = lm.positional_encoding.pe
        W.emb, W.pe = ptr(emb), ptr(pe.reshape(pe.shape[-2], pe.shape[-1]))
        W.final_ln_g, W.final_ln_b = ptr(enc.norm.norm.weight), ptr(enc.norm.norm.bias)
        o0, oln, o2 = lm.output_proj.layers[0], lm.output_proj.layers[1], lm.output_proj.layers[2]
        W.out0_w, W.out0_b = ptr(o0.w.weight), ptr(o0.w.bias)
        W.out_ln_g, W.out_ln_b = ptr(oln.norm.weight), ptr(oln.norm.bias)
        W.out2_w, W.out2_b = ptr(o2.w.weight), ptr(o2.w.bias)
        W.d_model, W.nhead = emb.shape[1], enc.layers[0].nhead
        W.d_ffn, W.n_layers, W.vocab = enc.layers[0].pos_ffn.ffn[0].weight.shape[0], len(enc.layers), o2.w.weight.shape[0]
        W.max_len, W.ffn_act = pe.shape[-2], enc.layers[0].pos_ffn.act_code
        W.normalize_before, W.pad_idx, W.ln_eps = int(enc.layers[0].normalize_before), 0, enc.norm.eps
        self.W, self.device = W, emb.device
        self.ready = _Ready(emb.device)
        self.key = self.source_key(lm)

    @staticmethod
    def source_key(lm):
        """``source_key`` of every source tensor (see DecoderHandle.source_key)."""
        return source_key(list(lm.parameters()) + [lm.positional_encoding.pe])

    def stale(self, lm):
        return self.source_key(lm) != self.key


def lm_prefix(handle: "LMHandle", tokens):
    """TransformerLM.forward: tokens [n,L] int32 -> logits [n,L,V] (KV-cached, causal, pad-0 keys masked)."""
    lib = load()
    _dev_ok(tokens)
    n, L = tokens.shape
    handle.ready.wait(tokens.device)
    nbytes = lib.sbk_lm_prefix_workspace_bytes(ctypes.byref(handle.W), n, L)
    ws = _Workspace(nbytes, tokens.device)
    out = torch.empty(n, L, handle.W.vocab, dtype=torch.float32, device=tokens.device)
    _chk(lib.sbk_lm_prefix_f32(ctypes.byref(handle.W), _p(tokens), ws.ptr, nbytes, _p(out), n, L, _stream(tokens)),
         "sbk_lm_prefix_f32")
    return out


def _fold_ln(w, b, gamma, beta):
    """(Wf, bf) with a preceding LayerNorm's affine folded in: Wf = W*gamma[k], bf = b + W.beta (fp64, rounded once)."""
    w64, g64, be64 = w.detach().double(), gamma.detach().double(), beta.detach().double()
    wf = (w64 * g64[None, :]).float().contiguous()
    bf = (b.detach().double() + w64 @ be64).float().contiguous()
    return wf, bf


def _host_flag(device):
    """A host int32 the C ABI takes as its "stop-rule polling allowed" argument (the library polls through its own
    pinned ring, csrc/search.hip AsyncPoll).  One per host thread, allocated once: pinning memory per search call costs
    a driver round trip per call."""
    t = getattr(_tls, "host_flag", None)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32)
        _tls.host_flag = t
    return t


def beam_search(handle: DecoderHandle, cfg: SearchConfig, enc, enc_len, ctc_w=None, ctc_b=None, utt_min_steps=None,
                utt_max_steps=None, want_longest=False):
    """Returns (tokens [B,max_steps] int32, lens [B] int32, scores [B], log_probs [B,max_steps],
    max_len [1] int32 (longest finished hypothesis), steps_run) -- plus longest [B] int32 with ``want_longest``.
    ``utt_min_steps`` / ``utt_max_steps`` (int32 [B] on the device): per-utterance step limits of a grouped search."""
    lib = load()
    _dev_ok(enc, enc_len, ctc_w, ctc_b, utt_min_steps, utt_max_steps)
    cfg.utt_min_steps = utt_min_steps.data_ptr() if utt_min_steps is not None else None
    cfg.utt_max_steps = utt_max_steps.data_ptr() if utt_max_steps is not None else None
    _f32(enc)
    B, T, _ = enc.shape
    dev = enc.device
    L = max(int(cfg.max_steps), 1)
    K = max(int(cfg.topk), 1)  # rows per utterance (return_topk)
    handle.ready.wait(dev)
    nbytes = lib.sbk_beam_search_workspace_bytes(ctypes.byref(handle.W), ctypes.byref(cfg), B, T)
    with _Workspace(nbytes, dev, per_stream=True) as ws:
        out_tok = torch.zeros(B * K, L, dtype=torch.int32, device=dev)
        out_len = torch.zeros(B * K, dtype=torch.int32, device=dev)
        out_score = torch.zeros(B * K, dtype=torch.float32, device=dev)
        out_lp = torch.zeros(B * K, L, dtype=torch.float32, device=dev)
        out_max = torch.zeros(1, dtype=torch.int32, device=dev)
        out_longest = torch.zeros(B, dtype=torch.int32, device=dev) if want_longest else None
        flag = _host_flag(dev)
        steps = c_int32(0)
        cfg.ctc_w3 = None
        if ctc_w is not None and F32X3 and ctc_w.dim() == 2 and ctc_w.is_contiguous() and _x3_shape(*ctc_w.shape):
            cfg.ctc_w3 = lp_weight(ctc_w, "x3").data_ptr()  # (cached with the parameter: the CTC head over B*T frames)
        _chk(lib.sbk_beam_search_f32(ctypes.byref(handle.W), ctypes.byref(cfg), _p(enc), _p(enc_len), _p(ctc_w), _p(ctc_b),
                                     ws.ptr, nbytes, _p(out_tok), _p(out_len), _p(out_score), _p(out_lp), _p(out_max),
                                     _p(out_longest), c_void_p(flag.data_ptr()), ctypes.byref(steps), B, T, _stream(enc)),
             "sbk_beam_search_f32")
    if want_longest:
        return out_tok, out_len, out_score, out_lp, out_max, steps.value, out_longest
    return out_tok, out_len, out_score, out_lp, out_max, steps.value


# SBK_WS_TRIM=1: an outgrown multi-GB search buffer is handed back to the driver (torch.cuda.empty_cache) instead of staying in
# its stream's pool.  OFF by default: on one box (profiles/r05_i_*) it took the bench's reserved memory from 81.5 to 67 GB but
# the headline from 11.7 K to 8.7-11.1 K audio-s/s -- the emptied pools are refilled by hipMalloc inside the next job.
WS_TRIM = os.environ.get("SBK_WS_TRIM", "0") != "0"
_SEARCH_WS = {}  # (device index, stream handle) -> [buffer, a host thread is enqueueing a search into it]
_SEARCH_WS_LOCK = threading.RLock()  # (re-entrant: a transcriber finalised by the cyclic GC inside an allocation made under the lock)


def _search_workspace(nbytes: int, dev):
    """The search workspace of the current stream: ONE grow-only buffer per (device, stream), reused by the searches that
    follow each other on that stream (stream order makes the reuse safe; the library joins its helper stream before it
    returns) and kept ACROSS the jobs of a transcriber (``release_search_workspaces``: when its streams retire).
    Rounds 3-4 kept it per (thread, stream) and dropped it after every job: the caching allocator then served a later, smaller
    request by splitting the cached block and a still later, larger one from a fresh segment -- 106-133 GB reserved for 62-71 GB
    allocated.  Returns (buffer, key); ``_search_workspace_done(key)`` when the library call has
    returned.  A second host thread that starts a search on the same stream meanwhile gets a private buffer (key None)."""
    if dev.type != "cuda":
        return torch.empty(nbytes, dtype=torch.uint8, device=dev), None
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    with _SEARCH_WS_LOCK:
        ent = _SEARCH_WS.get(key)
        if ent is not None and ent[1]:
            return torch.empty(nbytes, dtype=torch.uint8, device=dev), None
        if ent is None or ent[0].numel() < nbytes:
            grown = WS_TRIM and ent is not None and ent[0].numel() >= (256 << 20)
            _SEARCH_WS.pop(key, None)
            ent = None  # (the old block goes back to the allocator before the larger one is requested)
            if grown:
                # (opt-in, see WS_TRIM: a multi-GB block that has just been outgrown sits in this stream's pool for good -- no
                #  later request of the pool is that large, and another stream's pool cannot take it)
                torch.cuda.empty_cache()
            ent = _SEARCH_WS[key] = [torch.empty(nbytes + (nbytes >> 3), dtype=torch.uint8, device=dev), False]
        ent[1] = True
        return ent[0], key


def _search_workspace_done(key):
    if key is None:
        return
    with _SEARCH_WS_LOCK:
        ent = _SEARCH_WS.get(key)
        if ent is not None:
            ent[1] = False


def release_search_workspaces(streams=None):
    """Drop the cached search workspaces of the given ``torch.cuda.Stream`` objects (a ConcurrentTranscriber calls it for its
    worker streams when it is closed), or -- ``None`` -- of every stream no search is running on."""
    with _SEARCH_WS_LOCK:
        if streams is None:
            keys = [k for k, ent in _SEARCH_WS.items() if not ent[1]]
        else:
            keys = [(s.device.index, s.cuda_stream) for s in streams]
        for k in keys:
            ent = _SEARCH_WS.get(k)
            if ent is not None and not ent[1]:  # (a search of another owner of the same pooled handle is running on it: kept)
                _SEARCH_WS.pop(k, None)


def greedy_search(handle: DecoderHandle, enc, enc_len, min_steps, max_steps, bos, eos, check_every=8):
    """Returns (tokens [B,max_steps] int32 (EOS-latched), scores [B,max_steps], steps_run)."""
    lib = load()
    _dev_ok(enc, enc_len)
    B, T, _ = enc.shape
    dev = enc.device
    L = max(int(max_steps), 1)
    handle.ready.wait(dev)
    nbytes = lib.sbk_greedy_search_workspace_bytes(ctypes.byref(handle.W), B, T, max_steps)
    ws = _Workspace(nbytes, dev)
    out_tok = torch.zeros(B, L, dtype=torch.int32, device=dev)
    out_sc = torch.zeros(B, L, dtype=torch.float32, device=dev)
    flag = _host_flag(dev)
    steps = c_int32(0)
    _chk(lib.sbk_greedy_search_f32(ctypes.byref(handle.W), _p(enc), _p(enc_len), ws.ptr, nbytes,
                                   _p(out_tok), _p(out_sc), c_void_p(flag.data_ptr()), ctypes.byref(steps), B, T,
                                   int(min_steps), int(max_steps), int(bos), int(eos), int(check_every), _stream(enc)),
         "sbk_greedy_search_f32")
    return out_tok, out_sc, steps.value


def prompted_greedy_search(handle: DecoderHandle, enc, enc_len, prompt, max_new, eos, logit_bias=None, first_bias=None,
                           probe=None, check_every=8):
    """S2SWhisperGreedySearcher on the device: prompt [B,P] int32 primes the KV cache, then arg-max decoding with the
    additive [V] masks.  Returns (tokens [B,max_new] (EOS-latched), scores [B,max_new], steps_run, probe [B] | None);
    ``probe`` = (prompt position, token): softmax probability of the token at that position."""
    lib = load()
    _dev_ok(enc, enc_len, prompt, logit_bias, first_bias)
    B, T, _ = enc.shape
    P = prompt.shape[1]
    dev = enc.device
    L = max(int(max_new), 1)
    handle.ready.wait(enc.device)
    nbytes = lib.sbk_prompted_greedy_search_workspace_bytes(ctypes.byref(handle.W), B, T, P, int(max_new))
    ws = _Workspace(nbytes, dev)
    out_tok = torch.zeros(B, L, dtype=torch.int32, device=dev)
    out_sc = torch.zeros(B, L, dtype=torch.float32, device=dev)
    out_probe = torch.zeros(B, dtype=torch.float32, device=dev) if probe is not None else None
    flag = _host_flag(dev)
    steps = c_int32(0)
    _chk(lib.sbk_prompted_greedy_search_f32(
        ctypes.byref(handle.W), _p(enc), _p(enc_len), _p(prompt), P, _p(logit_bias), _p(first_bias),
        ws.ptr, nbytes, _p(out_tok), _p(out_sc), int(probe[0]) if probe else 0,
        int(probe[1]) if probe else 0, _p(out_probe), c_void_p(flag.data_ptr()), ctypes.byref(steps), B, T, int(max_new),
        int(eos), int(check_every), _stream(enc)), "sbk_prompted_greedy_search_f32")
    return out_tok, out_sc, steps.value, out_probe


def decoder_prefix(handle: DecoderHandle, tokens, enc, enc_len):
    """tokens [n,L] int32, enc [n,T,d] -> decoder.norm output [n,L,d] (KV-cached, teacher forced)."""
    lib = load()
    _dev_ok(tokens, enc, enc_len)
    n, L = tokens.shape
    T = enc.shape[1]
    handle.ready.wait(enc.device)
    nbytes = lib.sbk_decoder_prefix_workspace_bytes(ctypes.byref(handle.W), n, T, L)
    ws = _Workspace(nbytes, enc.device)
    pred = torch.empty(n, L, handle.W.d_model, dtype=torch.float32, device=enc.device)
    _chk(lib.sbk_decoder_prefix_f32(ctypes.byref(handle.W), _p(tokens), _p(enc), _p(enc_len), ws.ptr, nbytes, _p(pred), n, T, L,
                                    _stream(enc)), "sbk_decoder_prefix_f32")
    return pred


class CTCStepScorer:
    """The CTC prefix scorer as a per-step object (sbk_ctc_scorer_*: decoders/ctc.py:79-295 CTCPrefixScore).  ``log_probs``
    [B,T,V] = log_softmax(ctc_fc(enc)) -- the scorer takes ownership and converts it in place --, ``enc_len`` [B] int32 absolute
    lengths.  ``score(inp_tokens, step)`` -> psi - psi_prev [B*beam, V]; ``permute(parent, token, inp_tokens, step)`` moves the
    state to the hypotheses chosen by the beam update.  The beam width is fixed by the first ``score`` call."""

    def __init__(self, log_probs, enc_len, blank, eos, ctc_window_size=0):
        _dev_ok(log_probs, enc_len)
        _f32(log_probs)
        self.x, self.enc_len = log_probs, enc_len.to(torch.int32)
        self.B, self.T, self.V = log_probs.shape
        self.blank, self.eos, self.window = int(blank), int(eos), int(ctc_window_size)
        self.beam, self.ws, self.nbytes = 0, None, 0

    def _ready(self, beam):
        if self.beam == beam:
            return
        if self.beam:
            raise SbkError(f"CTCStepScorer: the beam width changed from {self.beam} to {beam} inside one utterance batch")
        lib = load()
        self.beam = beam
        self.nbytes = lib.sbk_ctc_scorer_workspace_bytes(self.B, self.T, self.V, beam)
        self.ws = _Workspace(self.nbytes, self.x.device)
        _chk(lib.sbk_ctc_scorer_reset_f32(_p(self.x), _p(self.enc_len), self.ws.ptr, self.nbytes, self.B,
                                          self.T, self.V, beam, self.blank, _stream(self.x)), "sbk_ctc_scorer_reset_f32")

    def score(self, inp_tokens, step, attn_window=None):
        n = inp_tokens.shape[0]
        if n % self.B:
            raise SbkError(f"CTCStepScorer: {n} hypotheses for {self.B} utterances")
        self._ready(n // self.B)
        tok = inp_tokens.to(torch.int32).contiguous()
        out = torch.empty(n, self.V, dtype=torch.float32, device=self.x.device)
        _chk(load().sbk_ctc_scorer_score_f32(_p(self.x), _p(self.enc_len), self.ws.ptr, self.nbytes, _p(tok),
                                             int(step), _p(attn_window), self.window if attn_window is not None else 0, _p(out), self.B,
                                             self.T, self.V, self.beam, self.blank, self.eos, _stream(self.x)), "sbk_ctc_scorer_score_f32")
        return out

    def permute(self, parent, token, parent_last_tok, step, attn_window=None):
        par, tk, last = (t.to(torch.int32).contiguous() for t in (parent, token, parent_last_tok))
        _chk(load().sbk_ctc_scorer_permute_f32(_p(self.x), self.ws.ptr, self.nbytes, _p(par), _p(tk), _p(last),
                                               int(step), _p(attn_window), self.window if attn_window is not None else 0, self.B, self.T,
                                               self.V, self.beam, self.blank, _stream(self.x)), "sbk_ctc_scorer_permute_f32")


def log_softmax(x, temperature=1.0, weight=1.0):
    lib = load()
    V = x.shape[-1]
    x2 = x.reshape(-1, V)
    _dev_ok(x2)
    out = torch.empty_like(x)
    _chk(lib.sbk_log_softmax_f32(_p(x2), _p(out), x2.shape[0], V, float(temperature), float(weight), _stream(x2)),
         "sbk_log_softmax_f32")
    return out


# ------------------------------------------------------------------ CTC decoding (csrc/ctc_decode.hip)
def _rel_len(rel_len, device):  # as the CTC decoders take it: fp32 [B] on ``device``, or None (every frame)
    return None if rel_len is None else rel_len.to(device=device, dtype=torch.float32).contiguous()


def ctc_greedy_decode(x, rel_len, blank):
    """x [B,T,V] fp32 -> (tokens [B,T] int32, count [B] int32): row b's first count[b] entries are its collapsed,
    blank-free arg-max path over int(round(rel_len[b] * T)) frames (rel_len None = every frame)."""
    lib = load()
    _f32(x)
    B, T, V = x.shape
    x = x.contiguous()
    rel = _rel_len(rel_len, x.device)
    _dev_ok(x, rel)
    tokens = torch.empty(B, T, dtype=torch.int32, device=x.device)
    count = torch.empty(B, dtype=torch.int32, device=x.device)
    _chk(lib.sbk_ctc_greedy_decode_f32(_p(x), _p(rel), _p(tokens), _p(count), B, T, V, int(blank), _stream(x)),
         "sbk_ctc_greedy_decode_f32")
    return tokens, count


def ctc_beam_search(x, rel_len, table, n_vocab, cfg, lm=None):
    """CTCBeamSearcher on the device.  x [B,T,V] fp32 log-probabilities, table [n_vocab,8] int32 (the token table of
    include/sbk.h), cfg a CTCBeamConfig -> (paths [B,topk,T] int32, scores [B,topk], count [B]).  With ``lm`` (an object
    whose ``tables(device)`` gives a CTCLMTables over device tensors: decoders/ngram.py) the n-gram model is fused into the
    search (sbk_ctc_beam_search_lm_f32) and the fused scores [B,topk] are returned as a fourth value."""
    lib = load()
    _f32(x)
    B, T, V = x.shape
    x = x.contiguous()
    rel = _rel_len(rel_len, x.device)
    table = table.to(device=x.device, dtype=torch.int32).contiguous()
    _dev_ok(x, rel, table)
    nbytes = lib.sbk_ctc_beam_search_workspace_bytes(B, T, V, cfg.beam_size, cfg.topk)
    ws = _Workspace(nbytes, x.device, align=16, floor=1)
    paths = torch.empty(B, max(cfg.topk, 1), T, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, max(cfg.topk, 1), dtype=torch.float32, device=x.device)
    count = torch.empty(B, dtype=torch.int32, device=x.device)
    if lm is not None:
        tabs = lm.tables(x.device)
        lm_scores = torch.empty_like(scores)
        _chk(lib.sbk_ctc_beam_search_lm_f32(_p(x), _p(rel), _p(table), int(n_vocab), ctypes.byref(cfg), ctypes.byref(tabs),
                                            ws.ptr, nbytes, _p(paths), _p(scores), _p(lm_scores), _p(count), B, T, V,
                                            _stream(x)), "sbk_ctc_beam_search_lm_f32")
        return paths, scores, count, lm_scores
    _chk(lib.sbk_ctc_beam_search_f32(_p(x), _p(rel), _p(table), int(n_vocab), ctypes.byref(cfg), ws.ptr, nbytes, _p(paths),
                                     _p(scores), _p(count), B, T, V, _stream(x)), "sbk_ctc_beam_search_f32")
    return paths, scores, count


# ------------------------------------------------------------------ transducer greedy decoding (csrc/transducer.hip)
def _fill_lstm_stack(W, what, emb, lstm_layers, ptr):
    """The part sbk_transducer_weights and sbk_rnnlm_weights share: the Embedding folded into layer 0's input weights (one
    sbk_gemm_nt_f32, on the current stream), the other LSTM matrices as they are.  Returns emb_ih [n_emb, 4H] = E . W_ih^T."""
    if not 1 <= len(lstm_layers) <= TRANSDUCER_MAX_LAYERS:
        raise SbkError(f"{what}: {len(lstm_layers)} LSTM layers (1..{TRANSDUCER_MAX_LAYERS} supported)")
    w_ih0 = lstm_layers[0][0].detach().float().contiguous()
    with precision_scope("fp32"):
        emb_ih = gemm_nt(emb.detach().float().contiguous(), w_ih0)
    W.emb_ih = ptr(emb_ih)
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(lstm_layers):
        if l > 0:
            W.w_ih[l] = ptr(w_ih)
        W.w_hh[l], W.b_ih[l], W.b_hh[l] = ptr(w_hh), ptr(b_ih), ptr(b_hh)
    W.n_layers, W.hidden, W.n_emb = len(lstm_layers), lstm_layers[0][1].shape[1], emb.shape[0]
    return emb_ih


class TransducerPrepared:
    """The prediction network, joint and classifier of a transducer in the layouts of sbk_transducer_weights (include/sbk.h):
    the Embedding folded into layer 0's input weights, the other matrices as they are.  Built once per set of weights; the
    tensors are kept alive here for as long as the struct points at them."""

    def __init__(self, emb, lstm_layers, proj_w, proj_b, out_w, out_b):
        """emb [n_emb, E]; lstm_layers: [(w_ih [4H, in], w_hh [4H, H], b_ih or None, b_hh or None)] * L;
        proj_w [J, H], proj_b [J] or None; out_w [V, J], out_b [V] or None (all fp32 on one device)."""
        self.W, self._keep = W, keep = TransducerWeights(), []
        ptr = _keeper(keep, strict=False)
        self.emb_ih = _fill_lstm_stack(W, "transducer", emb, lstm_layers, ptr)
        W.proj, W.proj_b, W.out, W.out_b = ptr(proj_w), ptr(proj_b), ptr(out_w), ptr(out_b)
        W.joint, W.vocab = proj_w.shape[0], out_w.shape[0]
        self.device = self.emb_ih.device


class RNNLMPrepared:
    """An RNNLM (lobes/models/RNNLM.py) in the layouts of sbk_rnnlm_weights (include/sbk.h): the Embedding folded into layer
    0's input weights, the other matrices as they are.  Built once per set of weights; the tensors are kept alive here for as
    long as the struct points at them."""

    def __init__(self, emb, lstm_layers, dnn_blocks, out_w, out_b, act):
        """emb [n_emb, E]; lstm_layers: [(w_ih [4H, in], w_hh [4H, H], b_ih or None, b_hh or None)] * L; dnn_blocks:
        [(w [D, in], b [D] or None, ln_weight [D], ln_bias [D], ln_eps)] * n_dnn; out_w [V, D], out_b [V] or None; act: one of
        ACT_LEAKY_RELU, ACT_RELU, ACT_GELU, ACT_TANH (all fp32 on one device)."""
        if not 1 <= len(dnn_blocks) <= RNNLM_MAX_DNN:
            raise SbkError(f"RNNLM: {len(dnn_blocks)} DNN blocks (1..{RNNLM_MAX_DNN} supported)")
        self.M, self._keep = M, keep = RNNLMWeights(), []
        ptr = _keeper(keep, strict=False)
        self.emb_ih = _fill_lstm_stack(M, "RNNLM", emb, lstm_layers, ptr)
        for i, (w, b, g, beta, eps) in enumerate(dnn_blocks):
            M.dnn_w[i], M.dnn_b[i], M.ln_g[i], M.ln_b[i], M.ln_eps[i] = ptr(w), ptr(b), ptr(g), ptr(beta), float(eps)
        M.out, M.out_b = ptr(out_w), ptr(out_b)
        M.n_dnn, M.dnn, M.vocab, M.act = len(dnn_blocks), out_w.shape[1], out_w.shape[0], int(act)
        self.device = self.emb_ih.device
        # (what one LM step reads: every matrix once, and one row of emb_ih)
        self.weight_bytes = 4 * sum(int(x.numel()) for x in keep) - 4 * int(self.emb_ih.numel()) + 4 * 4 * M.hidden


def lstm(x, layers, hx=None):
    """torch.nn.LSTM(batch_first=True, unidirectional) on the device: x [B,T,in]; layers [(w_ih, w_hh, b_ih, b_hh)] * L;
    hx (h0, c0) [L,B,H] or None -> (out [B,T,H], (h [L,B,H], c [L,B,H])).  Per layer: the input part of the gates for the
    whole sequence with sbk_gemm_nt_f32, then the recurrence with sbk_lstm_f32."""
    lib = load()
    _f32(x)
    B, T, _ = x.shape
    L, H = len(layers), layers[0][1].shape[1]
    if hx is None:
        h = torch.zeros(L, B, H, dtype=torch.float32, device=x.device)
        c = torch.zeros(L, B, H, dtype=torch.float32, device=x.device)
    else:
        h, c = (t.detach().float().contiguous().clone() for t in hx)
    out = x.contiguous()
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
        with precision_scope("fp32"):
            xp = gemm_nt(out, w_ih.detach().float().contiguous())
        w_hh = w_hh.detach().float().contiguous()
        b_ih = None if b_ih is None else b_ih.detach().float().contiguous()
        b_hh = None if b_hh is None else b_hh.detach().float().contiguous()
        y = torch.empty(B, T, H, dtype=torch.float32, device=x.device)
        hl, cl = h[l], c[l]  # (contiguous views of the state)
        _dev_ok(xp, w_hh, b_ih, b_hh, hl, cl, y)
        _chk(lib.sbk_lstm_f32(_p(xp), _p(w_hh), _p(b_ih), _p(b_hh), _p(hl), _p(cl), _p(y), B, T, H, _stream(xp)),
             "sbk_lstm_f32")
        out = y
    return out, (h, c)


def transducer_greedy(prep: TransducerPrepared, tn, out_pn, h, c, blank, max_symbols_per_step=5, start_from_blank=True,
                      act=ACT_GELU, frame_block=0):
    """sbk_transducer_greedy_f32: tn [B,T,J] fp32; the state out_pn [B,J], h / c [L,B,H] is read (unless start_from_blank)
    and overwritten in place with the final state.  -> (tokens [B, T*(S+1)] int32, count [B] int32, score [B] fp32)."""
    lib = load()
    _f32(tn)
    B, T, J = tn.shape
    tn = tn.contiguous()
    _dev_ok(tn, out_pn, h, c)
    cfg = TransducerConfig(blank=int(blank), max_symbols_per_step=int(max_symbols_per_step),
                           start_from_blank=1 if start_from_blank else 0, frame_block=int(frame_block), act=int(act))
    cap = T * (int(max_symbols_per_step) + 1)
    tokens = torch.empty(B, max(cap, 1), dtype=torch.int32, device=tn.device)
    count = torch.empty(B, dtype=torch.int32, device=tn.device)
    score = torch.empty(B, dtype=torch.float32, device=tn.device)
    _chk(lib.sbk_transducer_greedy_f32(ctypes.byref(prep.W), ctypes.byref(cfg), _p(tn), _p(out_pn), _p(h), _p(c), _p(tokens),
                                       _p(count), _p(score), B, T, _stream(tn)), "sbk_transducer_greedy_f32")
    return tokens, count, score


def transducer_beam_max_expansions(beam_size) -> int:
    """The default bound on the expansions of one frame of the transducer beam search."""
    return 4 * int(beam_size)


def transducer_beam_search(prep: TransducerPrepared, tn, blank, beam_size, nbest, state_beam=2.3, expand_beam=2.3,
                           max_expansions=None, max_tokens=None, act=ACT_GELU, lm: Optional["RNNLMPrepared"] = None,
                           lm_weight=0.0, return_lm_steps=False):
    """sbk_transducer_beam_search_f32: tn [B,T,J] fp32 -> (tokens [B,nbest,max_tokens] int32, length [B,nbest] int32,
    score [B,nbest] fp32 (logp_score / len(prediction)), count [B] int32, status [B] int32 (TBEAM_* bits), expansions [B]
    int32).  max_expansions: the bound on a frame's expansions (default 4 * beam_size); max_tokens: the room per hypothesis
    (default T * max_expansions, which no hypothesis can exceed).  The workspace is the search workspace of the current
    stream (grow-only, one per device and stream).  With ``lm`` (an RNNLMPrepared) the search is
    sbk_transducer_beam_search_lm_f32 with ``lm_weight`` (> 0; the entry refuses anything else); ``return_lm_steps`` then
    appends the LM steps each utterance took ([B] int32)."""
    lib = load()
    _f32(tn)
    B, T, J = tn.shape
    tn = tn.contiguous()
    _dev_ok(tn)
    if max_expansions is None:
        max_expansions = transducer_beam_max_expansions(beam_size)
    if max_tokens is None:
        max_tokens = T * int(max_expansions)
    cfg = TransducerBeamConfig(blank=int(blank), beam_size=int(beam_size), nbest=int(nbest), state_beam=float(state_beam),
                               expand_beam=float(expand_beam), max_expansions=int(max_expansions),
                               max_tokens=int(max_tokens), act=int(act))
    dev = tn.device
    tokens = torch.empty(B, max(cfg.nbest, 1), max(cfg.max_tokens, 1), dtype=torch.int32, device=dev)
    length = torch.empty(B, max(cfg.nbest, 1), dtype=torch.int32, device=dev)
    score = torch.empty(B, max(cfg.nbest, 1), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    if lm is None:
        if return_lm_steps:
            raise SbkError("transducer_beam_search: return_lm_steps without an LM")
        nbytes = lib.sbk_transducer_beam_workspace_bytes(ctypes.byref(prep.W), ctypes.byref(cfg), B, T)
    else:
        if lm.device != prep.device:
            raise SbkError(f"transducer_beam_search: the LM is prepared on {lm.device}, the network on {prep.device}")
        nbytes = lib.sbk_transducer_beam_lm_workspace_bytes(ctypes.byref(prep.W), ctypes.byref(lm.M), ctypes.byref(cfg), B, T)
    with _Workspace(nbytes, dev, align=16, floor=16, per_stream=True) as ws:
        # (a refused configuration gives 0 bytes above; the entry then reports the reason)
        if lm is None:
            _chk(lib.sbk_transducer_beam_search_f32(ctypes.byref(prep.W), ctypes.byref(cfg), _p(tn), ws.ptr, nbytes, _p(tokens),
                                                    _p(length), _p(score), _p(count), _p(status), B, T, _stream(tn)),
                 "sbk_transducer_beam_search_f32")
        else:
            _chk(lib.sbk_transducer_beam_search_lm_f32(ctypes.byref(prep.W), ctypes.byref(lm.M), float(lm_weight),
                                                       ctypes.byref(cfg), _p(tn), ws.ptr, nbytes, _p(tokens), _p(length),
                                                       _p(score), _p(count), _p(status), B, T, _stream(tn)),
                 "sbk_transducer_beam_search_lm_f32")
        expansions = ws.buf[ws.off:ws.off + 4 * B].view(torch.int32).clone()
        lm_steps = ws.buf[ws.off + 4 * B:ws.off + 8 * B].view(torch.int32).clone() if lm is not None else None
    ret = (tokens, length, score, count, status, expansions)
    return ret + (lm_steps,) if return_lm_steps else ret


# ------------------------------------------------------------------ HIP-event profiler
def prof_enable(on: bool):
    load().sbk_prof_enable(1 if on else 0)


def prof_reset():
    load().sbk_prof_reset()


def prof_report():
    """{kernel: dict(count, ms, flops, bytes)} for everything launched since prof_reset()."""
    lib = load()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.sbk_prof_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms, flops, nbytes = line.split()
        out[name] = dict(count=int(count), ms=float(ms), flops=float(flops), bytes=float(nbytes))
    return out
