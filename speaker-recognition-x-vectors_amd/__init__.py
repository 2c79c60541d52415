"""MI355X-native x-vector embedding extractor (TDNN x5 -> stats pooling -> affine).

Drop-in for the model surface of TorbenHellriegel/Speaker-Recognition-x-vectors
(`XVectorModel.forward / extract_x_vec / stat_pool`, reference main.py:23-94) backed by
hand-written gfx950 HIP kernels behind the C-ABI in include/xvec_hip.h.
"""
from . import synth  # noqa: F401  (numpy only)

__all__ = ["synth", "XVectorModel", "TdnnLayer", "get_time_context", "MfccFrontEnd", "PldaScorer", "hip", "extract",
           "frontend", "scoring", "plda", "PldaStats", "PLDA", "StatObject", "evaluate", "TrialList", "TrialResult",
           "evaluate_trials", "evaluate_all_pairs", "plda_score_stat_object", "augment", "WaveAugmenter", "AugmentPlan",
           "train", "XVectorTrainer", "tdnn_layer_train", "DeviceAdam", "sliding_windows", "plan_segment_calls", "snorm",
           "ScoreNormalizer", "CohortStats", "cohort_stats", "apply_norm", "lda", "LDA", "LdaStats", "EmbeddingTransform",
           "resample", "Resampler", "speed_perturb", "identify", "SpeakerModels", "SpeakerIdentifier", "enroll",
           "open_set_scores", "identification_rate", "diarize", "Diarizer", "Diarization", "Clustering", "cluster", "turns",
           "write_rttm", "vad", "VadCmvn", "energy_vad", "sliding_cmvn", "select_voiced", "speech_runs", "run_windows", "visualize",
           "Tsne", "tsne_map", "tsne_affinities", "pca_map", "scatter_maps", "calibrate", "Calibration", "ScoreCalibrator", "CalibrationReport",
           "fit_calibration", "fit_calibration_all_pairs", "cllr", "min_cllr", "pav_segments", "calibration_report", "report", "DetCurve",
           "TrialReport", "trial_map", "score_range", "score_images", "det_curve", "det_curve_all_pairs", "trial_report", "vbx", "Vbx",
           "VbxModel", "VbxResult", "der", "DerResult", "read_rttm", "fuse", "Term", "Fusion", "FusionResult", "ScoreFuser", "fit_fusion",
           "fit_fusion_all_pairs", "log_duration_terms", "row_quality", "col_quality", "bootstrap", "BootstrapResult",
           "BootstrapComparison", "bootstrap_trials", "bootstrap_all_pairs", "analyze", "ScoreSummary", "ScoreHistogram", "HardestTrials",
           "score_summary", "score_summary_all_pairs", "hardest_trials", "hardest_all_pairs", "confusable_pairs",
           "compare_speaker_results", "gmm", "DiagGmm", "GmmStats", "fit_ubm", "map_adapt", "linear_scores", "llr_scores",
           "frames_of"]


def __getattr__(name):
    # torch-dependent parts load lazily so that `synth` stays importable anywhere
    if name in ("XVectorModel", "TdnnLayer", "get_time_context", "sliding_windows", "plan_segment_calls"):
        from . import model
        return getattr(model, name)
    if name == "MfccFrontEnd":
        from . import frontend
        return frontend.MfccFrontEnd
    if name == "PldaScorer":
        from . import scoring
        return scoring.PldaScorer
    if name in ("PldaStats", "PLDA", "StatObject"):
        from . import plda
        return getattr(plda, name)
    if name in ("TrialList", "TrialResult", "evaluate_trials", "evaluate_all_pairs", "plda_score_stat_object"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("ScoreNormalizer", "CohortStats", "cohort_stats", "apply_norm"):
        from . import snorm
        return getattr(snorm, name)
    if name in ("LDA", "LdaStats", "EmbeddingTransform"):
        import importlib
        return getattr(importlib.import_module(".lda", __name__), name)
    if name in ("Resampler", "speed_perturb"):
        import importlib
        return getattr(importlib.import_module(".resample", __name__), name)
    if name in ("SpeakerModels", "SpeakerIdentifier", "enroll", "open_set_scores", "identification_rate"):
        import importlib
        return getattr(importlib.import_module(".identify", __name__), name)
    if name in ("Diarizer", "Diarization", "Clustering", "cluster", "turns", "write_rttm"):
        import importlib
        return getattr(importlib.import_module(".diarize", __name__), name)
    if name in ("VadCmvn", "energy_vad", "sliding_cmvn", "select_voiced", "speech_runs", "run_windows"):
        import importlib
        return getattr(importlib.import_module(".vad", __name__), name)
    if name in ("Tsne", "tsne_map", "tsne_affinities", "pca_map", "scatter_maps"):
        import importlib
        return getattr(importlib.import_module(".visualize", __name__), name)
    if name in ("Calibration", "ScoreCalibrator", "CalibrationReport", "fit_calibration", "fit_calibration_all_pairs", "cllr",
                "min_cllr", "pav_segments", "calibration_report"):
        import importlib
        return getattr(importlib.import_module(".calibrate", __name__), name)
    if name in ("DetCurve", "TrialReport", "trial_map", "score_range", "score_images", "det_curve", "det_curve_all_pairs",
                "trial_report"):
        import importlib
        return getattr(importlib.import_module(".report", __name__), name)
    if name in ("Vbx", "VbxModel", "VbxResult"):
        import importlib
        return getattr(importlib.import_module(".vbx", __name__), name)
    if name in ("DerResult", "read_rttm"):
        import importlib
        return getattr(importlib.import_module(".der", __name__), name)
    if name in ("Term", "Fusion", "FusionResult", "ScoreFuser", "fit_fusion", "fit_fusion_all_pairs", "log_duration_terms",
                "row_quality", "col_quality"):
        import importlib
        return getattr(importlib.import_module(".fuse", __name__), name)
    if name in ("BootstrapResult", "BootstrapComparison", "bootstrap_trials", "bootstrap_all_pairs"):
        import importlib
        return getattr(importlib.import_module(".bootstrap", __name__), name)
    if name in ("ScoreSummary", "ScoreHistogram", "HardestTrials", "score_summary", "score_summary_all_pairs", "hardest_trials",
                "hardest_all_pairs", "confusable_pairs", "compare_speaker_results"):
        import importlib
        return getattr(importlib.import_module(".analyze", __name__), name)
    if name in ("DiagGmm", "GmmStats", "fit_ubm", "map_adapt", "linear_scores", "llr_scores", "frames_of"):
        import importlib
        return getattr(importlib.import_module(".gmm", __name__), name)
    if name in ("WaveAugmenter", "AugmentPlan"):
        from . import augment
        return getattr(augment, name)
    if name in ("XVectorTrainer", "tdnn_layer_train", "DeviceAdam"):
        from . import train
        return getattr(train, name)
    if name in ("hip", "model", "extract", "frontend", "scoring", "plda", "evaluate", "augment", "train", "snorm", "lda", "resample", "identify",
                "diarize", "vad", "visualize", "calibrate", "report", "vbx", "der", "fuse", "bootstrap", "analyze", "gmm"):
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(name)
