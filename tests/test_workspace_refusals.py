"""What every C-ABI entry point with a (workspace, workspace_bytes) pair answers to a null workspace and to one a byte short of
the reported size: the return code and the text of its *_last_error().  The answers were recorded from the library before the
back ends moved onto one workspace_arg_ok (csrc/host_support.h) and must not move: the training units answer XVEC_ERR_ARG where
the others answer XVEC_ERR_WORKSPACE, t-SNE alone prefixes the call's name, and the older units fold the workspace into one
"null pointer" test.  Every call here fails its argument checks before the library touches a device; the entry points that take
an engine handle (xvec_forward, xvec_forward_packed, xvec_forward_segments, xvec_tdnn_layer, xvec_tdnn_pool_layer,
xvec_segment_layer) cannot get that far without one and are left out."""
import ctypes as C

import pytest

P, Q = 0x1000, 0x2000      # pointers that are never followed
WS, WSB = object(), object()      # where the row's workspace and its size go


def _i64(*v):
    return (C.c_int64 * len(v))(*v)


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _vad():
    from xvector_amd import hip
    return C.byref(hip.VadOptions(5.0, 0.5, 0.6, 0, 0))


def _cmvn():
    from xvector_amd import hip
    return C.byref(hip.CmvnOptions(1, 1, 0, 0))


_TDNN_FWD = (P, 1, 1, 1, P, P, 1, _i32(0), 1, None, None, 1e-5, P, None, None, None, WS, WSB, None)
_TDNN_BWD = (P, P, P, 1, 1, 1, P, 1, _i32(0), 1, None, None, None, 1e-5, None, P, P, None, None, WS, WSB, None)
_TAIL_FWD = (P, 1, 2, 1, P, P, 1, P, P, P, P, 1, P, P, P, P, P, P, WS, WSB, None)
_TAIL_BWD = (P, P, 1, 2, 1, P, 1, P, P, 1, P, P, P, P, P, None, P, P, P, P, P, P, WS, WSB, None)
_TDNN_SIZE = ("xvec_tdnn_train_workspace_bytes", (1, 1, 1, 1, _i32(0), 1))
_TAIL_SIZE = ("xvec_train_tail_workspace_bytes", (1, 2, 1, 1, 1))

# entry point: (its error channel, (the size query, its arguments), the smallest valid arguments)
CALLS = {
    "xvec_plda_score": ("score", ("xvec_score_workspace_bytes", (2, 0, 2)), (P, 2, None, 0, 2, P, P, P, 0.0, 1.0, P, WS, WSB, None)),
    "xvec_plda_score_lowrank": ("score", ("xvec_score_workspace_bytes", (2, 0, 2)),
                                (P, 2, None, 0, 2, 1, P, P, P, 0.0, 1.0, P, WS, WSB, None)),
    "xvec_cosine_score": ("score", ("xvec_score_workspace_bytes", (2, 0, 2)), (P, 2, None, 0, 2, P, WS, WSB, None)),
    "xvec_plda_stats": ("plda", ("xvec_plda_stats_workspace_bytes", (2, 2, 1)),
                        (P, 0, 2, 2, P, _i64(0, 2), 1, 1.0, P, P, P, P, P, WS, WSB, None)),
    "xvec_plda_em_products": ("plda", ("xvec_plda_em_workspace_bytes", (1, 1)), (P, P, P, P, P, 1, 2, 1, P, WS, WSB, None)),
    "xvec_eval_trials": ("eval", ("xvec_eval_workspace_bytes", (1,)),
                         (P, 1, 1, 1, None, None, P, 1, 1.0, 1.0, 0.05, P, WS, WSB, None)),
    "xvec_eval_all_pairs": ("eval", ("xvec_eval_workspace_bytes", (1,)), (P, 1, 1, 1, P, P, 0, 1.0, 1.0, 0.05, P, WS, WSB, None)),
    "xvec_eval_sorted_keys": ("eval", ("xvec_eval_workspace_bytes", (1,)), (P, 1, 1, 1, None, None, P, 1, P, P, WS, WSB, None)),
    "xvec_snorm_row_stats": ("snorm", ("xvec_snorm_workspace_bytes", (1, 1)), (P, 1, 1, 1, 0, None, P, P, P, P, WS, WSB, None)),
    "xvec_model_mean": ("ident", ("xvec_model_mean_workspace_bytes", (1,)), (P, 0, 1, 1, 1, P, _i64(0, 1), 1, P, WS, WSB, None)),
    "xvec_open_set_scores": ("ident", ("xvec_ident_workspace_bytes", (2, 1, 0)), (P, 1, 2, 1, 0.5, P, 1, WS, WSB, None)),
    # (two row blocks and the longest list: there the top-k plan, not the open-set one, is what xvec_ident_workspace_bytes reports)
    "xvec_identify_topk": ("ident", ("xvec_ident_workspace_bytes", (513, 64, 5)),
                           (P, 64, 513, 64, 5, 0.0, P, P, None, WS, WSB, None)),
    "xvec_ahc_cluster": ("diar", ("xvec_ahc_workspace_bytes", (_i64(0, 1), 1)),
                         (P, 1, _i64(0, 1), 1, 0.0, 0, None, P, P, None, None, None, WS, WSB, None)),
    "xvec_lda_stats": ("lda", ("xvec_lda_stats_workspace_bytes", (1, 1, 1)),
                       (P, 0, 1, 1, P, _i64(0, 1), 1, P, P, P, P, WS, WSB, None)),
    "xvec_embed_transform": ("lda", ("xvec_embed_transform_workspace_bytes", (1, 1, 1)),
                             (P, 0, 1, 1, 1, None, None, 1, 0, Q, 1, WS, WSB, None)),
    "xvec_aug_mix": ("aug", ("xvec_aug_mix_workspace_bytes", (1, 1, 0)),
                     (P, 1, 1, 1, P, 0, 1, 1, P, None, 0, None, 0, None, P, WS, WSB, None)),
    "xvec_aug_reverb": ("aug", ("xvec_aug_reverb_workspace_bytes", (1, 1, 1)), (P, 1, 1, 1, P, 1, 1, P, P, P, WS, WSB, None)),
    "xvec_resample": ("resample", ("xvec_resample_workspace_bytes", (1, 1)),
                      (P, 0, 1, 1, 1, None, 0, (C.c_double * 1)(1.0), 1, P, 2, 0, 0, P, 0, 1, 1, P, WS, WSB, None)),
    "xvec_cmvn_sliding": ("vad", ("xvec_vad_workspace_bytes", (1, 1)),
                          lambda: (P, 1, 1, 1, 1, 1, None, _cmvn(), P, 1, P, 1, 1, P, WS, WSB, None)),
    "xvec_vad_cmvn": ("vad", ("xvec_vad_workspace_bytes", (1, 1)),
                      lambda: (P, 1, 1, 1, 1, 1, None, _vad(), _cmvn(), 1, P, 1, P, None, P, 1, 1, P, WS, WSB, None)),
    "xvec_tsne_sqdist": ("tsne", ("xvec_tsne_workspace_bytes", (2, 1)), (P, 0, 2, 1, 1, 1, P, 2, WS, WSB, None)),
    "xvec_tsne_affinities": ("tsne", ("xvec_tsne_workspace_bytes", (2, 0)), (P, 2, 2, 1.0, P, 2, None, WS, WSB, None)),
    "xvec_tsne_steps": ("tsne", ("xvec_tsne_workspace_bytes", (2, 0)),
                        (P, 2, 2, 2, P, P, P, 2, 1, 12.0, 0.5, 50.0, 0.01, None, None, WS, WSB, None)),
    "xvec_tdnn_train_forward": ("train", _TDNN_SIZE, _TDNN_FWD),
    "xvec_tdnn_train_backward": ("train", _TDNN_SIZE, _TDNN_BWD),
    "xvec_tdnn_train_forward_ragged": ("train", _TDNN_SIZE, _TDNN_FWD + (P,)),
    "xvec_tdnn_train_backward_ragged": ("train", _TDNN_SIZE, _TDNN_BWD + (P,)),
    "xvec_tdnn_train_forward_dropout": ("train", _TDNN_SIZE, _TDNN_FWD + (None, 0.5, 1, 2)),
    "xvec_tdnn_train_backward_dropout": ("train", _TDNN_SIZE, _TDNN_BWD + (None, 0.5)),
    "xvec_train_tail_forward": ("train", _TAIL_SIZE, _TAIL_FWD),
    "xvec_train_tail_backward": ("train", _TAIL_SIZE, _TAIL_BWD),
    "xvec_train_tail_forward_ragged": ("train", _TAIL_SIZE, _TAIL_FWD + (P,)),
    "xvec_train_tail_backward_ragged": ("train", _TAIL_SIZE, _TAIL_BWD + (P,)),
}

# entry point: (the reported size, (code, text) for a null workspace, (code, text) for size - 1 bytes); 1 = XVEC_ERR_ARG,
# 4 = XVEC_ERR_WORKSPACE
RECORDED = {
    "xvec_plda_score": (768, (1, "null pointer"), (4, "workspace too small: 767 < 768 bytes")),
    "xvec_plda_score_lowrank": (768, (1, "null pointer"), (4, "workspace too small: 767 < 768 bytes")),
    "xvec_cosine_score": (768, (1, "null pointer"), (4, "workspace too small: 767 < 768 bytes")),
    "xvec_plda_stats": (33024, (1, "null pointer"), (4, "workspace too small: 33023 < 33024 bytes")),
    "xvec_plda_em_products": (512, (1, "null pointer"), (4, "workspace too small: 511 < 512 bytes")),
    "xvec_eval_trials": (3584, (1, "null pointer"), (4, "workspace too small: 3583 < 3584 bytes")),
    "xvec_eval_all_pairs": (3584, (1, "null pointer"), (4, "workspace too small: 3583 < 3584 bytes")),
    "xvec_eval_sorted_keys": (3584, (1, "null pointer"), (4, "workspace too small: 3583 < 3584 bytes")),
    "xvec_snorm_row_stats": (256, (1, "null pointer: workspace"), (4, "workspace too small: 255 < 256 bytes")),
    "xvec_model_mean": (256, (1, "null pointer"), (4, "workspace too small: 255 < 256 bytes")),
    "xvec_open_set_scores": (768, (1, "null pointer: workspace"), (4, "workspace too small: 767 < 768 bytes")),
    "xvec_identify_topk": (24576, (1, "null pointer: workspace"), (4, "workspace too small: 24575 < 24576 bytes")),
    "xvec_ahc_cluster": (1536, (1, "null pointer: workspace"), (4, "workspace too small: 1535 < 1536 bytes")),
    "xvec_lda_stats": (33536, (1, "null pointer"), (4, "workspace too small: 33535 < 33536 bytes")),
    "xvec_embed_transform": (256, (1, "null pointer"), (4, "workspace too small: 255 < 256 bytes")),
    "xvec_aug_mix": (512, (1, "null pointer: pool / src_len / status / workspace"), (4, "workspace too small: 511 < 512 bytes")),
    "xvec_aug_reverb": (512, (1, "null pointer: rirs / rir_len / rir_of_utt / status / workspace"), (4, "workspace too small: 511 < 512 bytes")),
    "xvec_resample": (256, (1, "null pointer: workspace"), (4, "workspace too small: 255 < 256 bytes")),
    "xvec_cmvn_sliding": (512, (1, "null pointer: workspace"), (4, "workspace too small: 511 < 512 bytes")),
    "xvec_vad_cmvn": (512, (1, "null pointer: workspace"), (4, "workspace too small: 511 < 512 bytes")),
    "xvec_tsne_sqdist": (1792, (1, "xvec_tsne_sqdist: null pointer: workspace"), (4, "workspace too small: 1791 < 1792 bytes")),
    "xvec_tsne_affinities": (1536, (1, "xvec_tsne_affinities: null pointer: workspace"), (4, "workspace too small: 1535 < 1536 bytes")),
    "xvec_tsne_steps": (1536, (1, "xvec_tsne_steps: null pointer: workspace"), (4, "workspace too small: 1535 < 1536 bytes")),
    "xvec_tdnn_train_forward": (512, (1, "null pointer: workspace"), (1, "workspace too small: 511 < 512 bytes")),
    "xvec_tdnn_train_backward": (512, (1, "null pointer: workspace"), (1, "workspace too small: 511 < 512 bytes")),
    "xvec_tdnn_train_forward_ragged": (512, (1, "null pointer: workspace"), (1, "workspace too small: 511 < 512 bytes")),
    "xvec_tdnn_train_backward_ragged": (512, (1, "null pointer: workspace"), (1, "workspace too small: 511 < 512 bytes")),
    "xvec_tdnn_train_forward_dropout": (512, (1, "null pointer: workspace"), (1, "workspace too small: 511 < 512 bytes")),
    "xvec_tdnn_train_backward_dropout": (512, (1, "null pointer: workspace"), (1, "workspace too small: 511 < 512 bytes")),
    "xvec_train_tail_forward": (1536, (1, "null pointer: workspace"), (1, "workspace too small: 1535 < 1536 bytes")),
    "xvec_train_tail_backward": (1536, (1, "null pointer: workspace"), (1, "workspace too small: 1535 < 1536 bytes")),
    "xvec_train_tail_forward_ragged": (1536, (1, "null pointer: workspace"), (1, "workspace too small: 1535 < 1536 bytes")),
    "xvec_train_tail_backward_ragged": (1536, (1, "null pointer: workspace"), (1, "workspace too small: 1535 < 1536 bytes")),
}


def answer(name, ws, size_delta):
    """(the reported size, the return code, the channel's text) of `name` on its smallest valid arguments with workspace `ws`
    of the reported size + size_delta bytes."""
    from xvector_amd import hip
    channel, (size_fn, size_args), args = CALLS[name]
    need = getattr(hip.lib, size_fn)(*size_args)
    args = args() if callable(args) else args
    rc = getattr(hip.lib, name)(*[ws if a is WS else need + size_delta if a is WSB else a for a in args])
    return need, rc, getattr(hip.lib, f"xvec_{channel}_last_error")().decode()


def _entry_points_with_a_workspace_and_no_handle():
    from xvector_amd import hip
    takes = {n for n, (_, a) in hip._SIGS.items() if any(x is C.c_size_t and a[i - 1] is C.c_void_p for i, x in enumerate(a))}
    with_handle = {"xvec_forward", "xvec_forward_packed", "xvec_forward_segments", "xvec_tdnn_layer", "xvec_tdnn_pool_layer",
                   "xvec_segment_layer"}
    return takes - with_handle


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_and_short_workspaces_are_refused_as_recorded(name):
    assert _entry_points_with_a_workspace_and_no_handle() == set(CALLS) == set(RECORDED)      # (no row is missing)
    need, null, short = RECORDED[name]
    assert need >= 256 and need % 256 == 0
    assert answer(name, None, 0) == (need, *null)
    assert answer(name, P, -1) == (need, *short)
