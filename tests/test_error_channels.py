"""CPU-only: the score, PLDA, eval and MFCC error channels of the library are four separate texts, each per thread
(include/xvec_score.h, xvec_plda.h, xvec_eval.h, xvec_hip.h).  They share one type on the C++ side
(csrc/host_support.h); this pins that they do not share one buffer.  Every error provoked here is an argument check
that returns before the library touches a device."""
import threading


def _provokers(hip):
    lib = hip.lib
    return {
        "score": (lambda: lib.xvec_gemm_nt_f64(None, 0, None, 0, -1, 0, 1, None, None, 0.0, 1.0, None, 0, None),
                  lib.xvec_score_last_error, "bad GEMM shape M=-1 N=0 K=1"),
        "plda": (lambda: lib.xvec_plda_stats(None, hip.PLDA_X_F64, 1, 4, None, None, 1, 1.0, None, None, None, None, None,
                                             None, 0, None),
                 lib.xvec_plda_last_error, "need at least two training vectors (n = 1)"),
        "eval": (lambda: lib.xvec_eval_trials(None, 0, 0, 0, None, None, None, 0, 1.0, 1.0, 0.5, None, None, 0, None),
                 lib.xvec_eval_last_error, "n_trials = 0: need at least one trial"),
        "mfcc": (lambda: lib.xvec_mfcc_create(None, None),
                 lib.xvec_mfcc_last_error, "null argument"),
    }


def test_error_channels_are_separate_and_per_thread():
    from xvector_amd import hip
    chans = _provokers(hip)
    texts = [want for _, _, want in chans.values()]
    assert len(set(texts)) == len(texts)                     # four different messages: a shared buffer cannot hold them all
    raised = []
    for name, (provoke, last_error, want) in chans.items():
        assert provoke() == hip.ERR_ARG, name
        raised.append(name)
        for other in raised:                                 # its own message, and the earlier channels still hold theirs
            assert chans[other][1]().decode() == chans[other][2], (name, other)

    seen = {}
    t = threading.Thread(target=lambda: seen.update({n: c[1]().decode() for n, c in chans.items()}))
    t.start()
    t.join()
    assert seen == {n: "" for n in chans}                    # a thread that has made no failing call reads nothing
    for name, (_, last_error, want) in chans.items():        # ... and reading there changed nothing here
        assert last_error().decode() == want, name
