"""ctypes mirror of include/stratum_hip.h (the C ABI of libstratum_hip.so).

Field order and types must match the header exactly; tests/test_abi.py checks sizes and
offsets against the compiled library (sdsp_abi_layout probe).
"""
import ctypes as C

u8, i8, i32, u32, u64, f32 = C.c_uint8, C.c_int8, C.c_int32, C.c_uint32, C.c_uint64, C.c_float


class SdspConfig(C.Structure):
    """AnalysisConfig, reference src/config.rs:8-592."""

    _fields_ = [
        ("min_amplitude_db", f32),
        ("normalization", i32),
        ("enable_normalization", u8),
        ("enable_silence_trimming", u8),
        ("enable_onset_consensus", u8),
        ("onset_threshold_percentile", f32),
        ("onset_consensus_tolerance_ms", u32),
        ("onset_consensus_weights", f32 * 4),
        ("enable_hpss_onsets", u8),
        ("hpss_margin", u64),
        ("force_legacy_bpm", u8),
        ("enable_bpm_fusion", u8),
        ("enable_legacy_bpm_guardrails", u8),
        ("enable_tempogram_multi_resolution", u8),
        ("tempogram_multi_res_top_k", u64),
        ("tempogram_multi_res_w512", f32),
        ("tempogram_multi_res_w256", f32),
        ("tempogram_multi_res_w1024", f32),
        ("tempogram_multi_res_structural_discount", f32),
        ("tempogram_multi_res_double_time_512_factor", f32),
        ("tempogram_multi_res_margin_threshold", f32),
        ("tempogram_multi_res_use_human_prior", u8),
        ("enable_tempogram_percussive_fallback", u8),
        ("enable_tempogram_band_fusion", u8),
        ("tempogram_band_low_max_hz", f32),
        ("tempogram_band_mid_max_hz", f32),
        ("tempogram_band_high_max_hz", f32),
        ("tempogram_band_w_full", f32),
        ("tempogram_band_w_low", f32),
        ("tempogram_band_w_mid", f32),
        ("tempogram_band_w_high", f32),
        ("tempogram_band_seed_only", u8),
        ("tempogram_band_support_threshold", f32),
        ("tempogram_band_consensus_bonus", f32),
        ("tempogram_novelty_w_spectral", f32),
        ("tempogram_novelty_w_energy", f32),
        ("tempogram_novelty_w_hfc", f32),
        ("tempogram_novelty_local_mean_window", u64),
        ("tempogram_novelty_smooth_window", u64),
        ("has_debug_track_id", u8),
        ("debug_track_id", u32),
        ("has_debug_gt_bpm", u8),
        ("debug_gt_bpm", f32),
        ("debug_top_n", u64),
        ("enable_tempogram_mel_novelty", u8),
        ("tempogram_mel_n_mels", u64),
        ("tempogram_mel_fmin_hz", f32),
        ("tempogram_mel_fmax_hz", f32),
        ("tempogram_mel_max_filter_bins", u64),
        ("tempogram_mel_weight", f32),
        ("tempogram_superflux_max_filter_bins", u64),
        ("emit_tempogram_candidates", u8),
        ("tempogram_candidates_top_n", u64),
        ("legacy_bpm_preferred_min", f32),
        ("legacy_bpm_preferred_max", f32),
        ("legacy_bpm_soft_min", f32),
        ("legacy_bpm_soft_max", f32),
        ("legacy_bpm_conf_mul_preferred", f32),
        ("legacy_bpm_conf_mul_soft", f32),
        ("legacy_bpm_conf_mul_extreme", f32),
        ("min_bpm", f32),
        ("max_bpm", f32),
        ("bpm_resolution", f32),
        ("frame_size", u64),
        ("hop_size", u64),
        ("center_frequency", f32),
        ("soft_chroma_mapping", u8),
        ("soft_mapping_sigma", f32),
        ("chroma_sharpening_power", f32),
        ("enable_key_spectrogram_time_smoothing", u8),
        ("key_spectrogram_smooth_margin", u64),
        ("enable_key_frame_weighting", u8),
        ("key_min_tonalness", f32),
        ("key_tonalness_power", f32),
        ("key_energy_power", f32),
        ("enable_key_harmonic_mask", u8),
        ("key_harmonic_mask_power", f32),
        ("enable_key_hpss_harmonic", u8),
        ("key_hpss_frame_step", u64),
        ("key_hpss_time_margin", u64),
        ("key_hpss_freq_margin", u64),
        ("key_hpss_mask_power", f32),
        ("enable_key_stft_override", u8),
        ("key_stft_frame_size", u64),
        ("key_stft_hop_size", u64),
        ("enable_key_log_frequency", u8),
        ("enable_key_beat_synchronous", u8),
        ("enable_key_multi_scale", u8),
        ("key_template_set", i32),
        ("enable_key_ensemble", u8),
        ("key_ensemble_kk_weight", f32),
        ("key_ensemble_temperley_weight", f32),
        ("enable_key_median", u8),
        ("key_median_segment_length_frames", u64),
        ("key_median_segment_hop_frames", u64),
        ("key_median_min_segments", u64),
        ("key_multi_scale_lengths", C.POINTER(u64)),
        ("key_multi_scale_lengths_len", u64),
        ("key_multi_scale_hop", u64),
        ("key_multi_scale_min_clarity", f32),
        ("key_multi_scale_weights", C.POINTER(f32)),
        ("key_multi_scale_weights_len", u64),
        ("enable_key_tuning_compensation", u8),
        ("key_tuning_max_abs_semitones", f32),
        ("key_tuning_frame_step", u64),
        ("key_tuning_peak_rel_threshold", f32),
        ("enable_key_edge_trim", u8),
        ("key_edge_trim_fraction", f32),
        ("enable_key_segment_voting", u8),
        ("key_segment_len_frames", u64),
        ("key_segment_hop_frames", u64),
        ("key_segment_min_clarity", f32),
        ("enable_key_mode_heuristic", u8),
        ("key_mode_third_ratio_margin", f32),
        ("key_mode_flip_min_score_ratio", f32),
        ("enable_key_hpcp", u8),
        ("key_hpcp_peaks_per_frame", u64),
        ("key_hpcp_num_harmonics", u64),
        ("key_hpcp_harmonic_decay", f32),
        ("key_hpcp_mag_power", f32),
        ("enable_key_hpcp_whitening", u8),
        ("key_hpcp_whitening_smooth_bins", u64),
        ("enable_key_hpcp_bass_blend", u8),
        ("key_hpcp_bass_fmin_hz", f32),
        ("key_hpcp_bass_fmax_hz", f32),
        ("key_hpcp_bass_weight", f32),
        ("enable_key_minor_harmonic_bonus", u8),
        ("key_minor_leading_tone_bonus_weight", f32),
        ("enable_ml_refinement", u8),
    ]


class SdspTempoCandidate(C.Structure):
    _fields_ = [("bpm", f32), ("score", f32), ("fft_norm", f32), ("autocorr_norm", f32), ("selected", u8)]


class SdspResult(C.Structure):
    """AnalysisResult + metadata, reference src/analysis/result.rs:144-263."""

    _fields_ = [
        ("bpm", f32),
        ("bpm_confidence", f32),
        ("key_mode", i32),
        ("key_tonic", u32),
        ("key_confidence", f32),
        ("key_clarity", f32),
        ("beats", C.POINTER(f32)),
        ("n_beats", u64),
        ("downbeats", C.POINTER(f32)),
        ("n_downbeats", u64),
        ("bars", C.POINTER(f32)),
        ("n_bars", u64),
        ("grid_stability", f32),
        ("duration_seconds", f32),
        ("sample_rate", u32),
        ("processing_time_ms", f32),
        ("algorithm_version", C.c_char * 16),
        ("onset_method_consensus", f32),
        ("methods_used", u32),
        ("flags", u32),
        ("warnings", C.POINTER(C.c_char_p)),
        ("n_warnings", u64),
        ("tempogram_candidates", C.POINTER(SdspTempoCandidate)),
        ("n_tempogram_candidates", u64),
        ("has_tempogram_candidates", i8),
        ("tempogram_multi_res_triggered", i8),
        ("tempogram_multi_res_used", i8),
        ("tempogram_percussive_triggered", i8),
        ("tempogram_percussive_used", i8),
        ("status", i32),
        ("error_message", C.c_char * 256),
    ]


class SdspStageTimes(C.Structure):
    _fields_ = [
        ("stft2048_ms", C.c_double),
        ("stft8192_ms", C.c_double),
        ("features_ms", C.c_double),
        ("tempogram_ms", C.c_double),
        ("key_ms", C.c_double),
        ("beat_ms", C.c_double),
        ("total_ms", C.c_double),
        ("stft2048_launches", u64),
        ("stft8192_launches", u64),
        ("stft2048_bytes", C.c_double),
        ("stft8192_bytes", C.c_double),
        ("stft2048_frames", u64),
        ("stft8192_frames", u64),
        ("key_reruns", u64),
        ("rerun_ms", C.c_double),
    ]


class SdspFlacDecodeStats(C.Structure):
    """sdsp_flac_decode_stats: counters and phase times of the last sdsp_decode_flac_batch_device call."""

    _fields_ = [
        ("files", u64),
        ("device_files", u64),
        ("host_fallback_files", u64),
        ("error_files", u64),
        ("candidates", u64),
        ("frames_accepted", u64),
        ("frames_rejected", u64),
        ("bytes_in", u64),
        ("samples_out", u64),
        ("scan_ms", C.c_double),
        ("frames_ms", C.c_double),
        ("chain_ms", C.c_double),
        ("gather_ms", C.c_double),
        ("total_ms", C.c_double),
    ]


class SdspDecodeStats(C.Structure):
    """sdsp_decode_stats: counters and phase times of the last sdsp_decode_batch_device call."""

    _fields_ = [
        ("files", u64),
        ("device_files", u64),
        ("host_fallback_files", u64),
        ("error_files", u64),
        ("flac_files", u64),
        ("alac_files", u64),
        ("pcm_files", u64),
        ("alac_packets", u64),
        ("alac_packets_decoded", u64),
        ("alac_packets_skipped", u64),
        ("bytes_in", u64),
        ("samples_out", u64),
        ("upload_ms", C.c_double),
        ("flac_ms", C.c_double),
        ("alac_ms", C.c_double),
        ("pcm_ms", C.c_double),
        ("gather_ms", C.c_double),
        ("total_ms", C.c_double),
    ]


class SdspAudioDecodeStats(C.Structure):
    """sdsp_audio_decode_stats: counters and phase times of the last sdsp_decode_audio_batch_device call."""

    _fields_ = [
        ("files", u64),
        ("device_files", u64),
        ("host_fallback_files", u64),
        ("error_files", u64),
        ("flac_files", u64),
        ("alac_files", u64),
        ("pcm_files", u64),
        ("vorbis_files", u64),
        ("alac_packets", u64),
        ("alac_packets_decoded", u64),
        ("alac_packets_skipped", u64),
        ("vorbis_packets", u64),
        ("vorbis_packets_zeroed", u64),
        ("bytes_in", u64),
        ("samples_out", u64),
        ("upload_ms", C.c_double),
        ("flac_ms", C.c_double),
        ("alac_ms", C.c_double),
        ("pcm_ms", C.c_double),
        ("gather_ms", C.c_double),
        ("vorbis_ms", C.c_double),
        ("total_ms", C.c_double),
    ]


class SdspConfidence(C.Structure):
    _fields_ = [
        ("bpm_confidence", f32),
        ("key_confidence", f32),
        ("grid_stability", f32),
        ("overall_confidence", f32),
        ("n_flags", u32),
        ("flag_list", C.c_int32 * 8),
    ]


class SdspOverviewRequest(C.Structure):
    """sdsp_overview_request: exactly one of columns / frames_per_column is non-zero."""

    _fields_ = [
        ("columns", u32),
        ("frames_per_column", u32),
        ("low_max_hz", f32),
        ("mid_max_hz", f32),
    ]


class SdspOverview(C.Structure):
    """sdsp_overview: one track's overview envelope (library-owned arrays, n_columns each)."""

    _fields_ = [
        ("n_columns", u64),
        ("n_frames", u64),
        ("first_sample", u64),
        ("n_samples", u64),
        ("frame_size", u32),
        ("hop_size", u32),
        ("band_bins", u32 * 2),
        ("smin", C.POINTER(f32)),
        ("smax", C.POINTER(f32)),
        ("low", C.POINTER(f32)),
        ("mid", C.POINTER(f32)),
        ("high", C.POINTER(f32)),
        ("status", C.c_int32),
    ]


class SdspDebugOverviewTimes(C.Structure):
    """sdsp_debug_overview_times (include/stratum_hip_debug.h)."""

    _fields_ = [
        ("sample_ms", C.c_double),
        ("band_ms", C.c_double),
        ("sample_bytes", C.c_double),
        ("band_bytes", C.c_double),
        ("columns", u64),
        ("sub_batches", u64),
    ]


class SdspKeyTimelineRequest(C.Structure):
    """sdsp_key_timeline_request: the seconds form or the frames form, exactly one."""

    _fields_ = [
        ("segment_seconds", f32),
        ("overlap_seconds", f32),
        ("segment_frames", u32),
        ("hop_frames", u32),
        ("min_change_confidence", f32),
    ]


class SdspKeySegment(C.Structure):
    """sdsp_key_segment: detect_key over one segment of the smoothed chroma rows."""

    _fields_ = [
        ("start_frame", u64),
        ("timestamp", f32),
        ("key", C.c_int32),
        ("confidence", f32),
        ("clarity", f32),
        ("top_keys", C.c_int32 * 3),
        ("top_scores", f32 * 3),
    ]


class SdspKeyChange(C.Structure):
    """sdsp_key_change: a reported change between segments segment - 1 and segment."""

    _fields_ = [
        ("segment", u64),
        ("timestamp", f32),
        ("from_key", C.c_int32),
        ("to_key", C.c_int32),
        ("confidence", f32),
    ]


class SdspKeyTimeline(C.Structure):
    """sdsp_key_timeline: one track's segments, primary key and changes (library-owned arrays)."""

    _fields_ = [
        ("n_segments", u64),
        ("n_changes", u64),
        ("n_frames", u64),
        ("first_sample", u64),
        ("segment_frames", u32),
        ("hop_frames", u32),
        ("frame_size", u32),
        ("hop_size", u32),
        ("primary_key", C.c_int32),
        ("primary_confidence", f32),
        ("primary_count", u64),
        ("segments", C.POINTER(SdspKeySegment)),
        ("changes", C.POINTER(SdspKeyChange)),
        ("status", C.c_int32),
    ]


LEVELS_PEAK, LEVELS_RMS, LEVELS_LOUDNESS, LEVELS_SILENCE_MAP = 1, 2, 4, 8  # enum sdsp_levels_what
LEVELS_BITS = {"peak": LEVELS_PEAK, "rms": LEVELS_RMS, "loudness": LEVELS_LOUDNESS, "silence": LEVELS_SILENCE_MAP}


class SdspLevelsRequest(C.Structure):
    """sdsp_levels_request: `what` is a mask of sdsp_levels_what bits."""

    _fields_ = [("what", u32)]


class SdspLoudness(C.Structure):
    """sdsp_loudness: the reference's LoudnessMetadata of one normalisation method."""

    _fields_ = [
        ("status", C.c_int32),
        ("measured", C.c_int8),
        ("has_lufs", C.c_int8),
        ("measured_lufs", f32),
        ("peak_db", f32),
        ("rms_db", f32),
        ("gain_db", f32),
        ("gain", f32),
    ]


class SdspSilenceRegion(C.Structure):
    """sdsp_silence_region: [start_sample, end_sample) in the caller's track."""

    _fields_ = [("start_sample", u64), ("end_sample", u64), ("duration_seconds", f32)]


class SdspLevels(C.Structure):
    """sdsp_levels: one track's loudness metadata per method and its silence map (library-owned)."""

    _fields_ = [
        ("method", SdspLoudness * 3),
        ("applied_gain", f32),
        ("n_samples", u64),
        ("trim_start", u64),
        ("trim_end", u64),
        ("frame_size", u32),
        ("threshold_db", f32),
        ("n_regions", u64),
        ("regions", C.POINTER(SdspSilenceRegion)),
        ("status", C.c_int32),
    ]


TEMPO_MAP_SEGMENTS, TEMPO_MAP_ONSETS = 1, 2  # enum sdsp_tempo_map_what
TEMPO_MAP_BITS = {"segments": TEMPO_MAP_SEGMENTS, "onsets": TEMPO_MAP_ONSETS}


class SdspTempoMapRequest(C.Structure):
    """sdsp_tempo_map_request: `what` is a mask of sdsp_tempo_map_what bits."""

    _fields_ = [("what", u32)]


class SdspTempoSegment(C.Structure):
    """sdsp_tempo_segment: one TempoSegment and what the Bayesian refinement did with it."""

    _fields_ = [
        ("start_time", f32),
        ("end_time", f32),
        ("bpm", f32),
        ("confidence", f32),
        ("is_variable", C.c_uint8),
        ("updated", C.c_uint8),
        ("n_onsets", u32),
        ("updated_bpm", f32),
        ("updated_confidence", f32),
        ("n_beats", u32),
    ]


class SdspTempoMap(C.Structure):
    """sdsp_tempo_map: one track's tempo segments, time signature and consensus onsets (library-owned)."""

    _fields_ = [
        ("status", C.c_int32),
        ("has_grid", C.c_int8),
        ("has_variation", C.c_int8),
        ("refined", C.c_int8),
        ("time_signature_scored", C.c_int8),
        ("nominal_bpm", f32),
        ("nominal_confidence", f32),
        ("hmm_beats", u32),
        ("beats_per_bar", u32),
        ("time_signature_confidence", f32),
        ("time_signature_scores", f32 * 3),
        ("first_sample", u64),
        ("n_segments", u64),
        ("segments", C.POINTER(SdspTempoSegment)),
        ("n_onsets", u64),
        ("onsets", C.POINTER(u32)),
    ]


class SdspDebugTempoMapTimes(C.Structure):
    """sdsp_debug_tempo_map_times (include/stratum_hip_debug.h)."""

    _fields_ = [("map_ms", C.c_double), ("beat_ms", C.c_double), ("tracks", u64)]


SECTIONS_LIST, SECTIONS_CURVE = 1, 2  # enum sdsp_sections_what
SECTIONS_BITS = {"list": SECTIONS_LIST, "curve": SECTIONS_CURVE}


class SdspSectionsRequest(C.Structure):
    """sdsp_sections_request: the cell (seconds or samples form, exactly one), K, G and the weights."""

    _fields_ = [
        ("what", u32),
        ("cell_seconds", f32),
        ("cell_samples", u64),
        ("kernel_cells", u32),
        ("min_gap_cells", u32),
        ("energy_weight", f32),
        ("min_strength", f32),
        ("snap_seconds", f32),
    ]


class SdspSection(C.Structure):
    """sdsp_section: one run of cells between two boundaries."""

    _fields_ = [
        ("start_cell", u64),
        ("end_cell", u64),
        ("start_time", f32),
        ("end_time", f32),
        ("strength", f32),
        ("mean_energy", f32),
        ("relative_energy", f32),
        ("snapped_time", f32),
        ("downbeat", C.c_int32),
    ]


class SdspSections(C.Structure):
    """sdsp_sections: one track's sections and curves (library-owned arrays)."""

    _fields_ = [
        ("status", C.c_int32),
        ("n_cells", u64),
        ("cell_samples", u64),
        ("first_sample", u64),
        ("gmax", f32),
        ("nmax", f32),
        ("n_sections", u64),
        ("sections", C.POINTER(SdspSection)),
        ("n_curve", u64),
        ("novelty", C.POINTER(f32)),
        ("energy", C.POINTER(f32)),
    ]


class SdspDebugSectionsOut(C.Structure):
    """sdsp_debug_sections_out (include/stratum_hip_debug.h): caller-owned arrays."""

    _fields_ = [
        ("cell_capacity", u64),
        ("n_cells", C.POINTER(u64)),
        ("m", C.POINTER(f32)),
        ("g", C.POINTER(f32)),
        ("novelty", C.POINTER(f32)),
        ("boundary", C.POINTER(C.c_uint8)),
    ]


class SdspDebugSectionsTimes(C.Structure):
    """sdsp_debug_sections_times (include/stratum_hip_debug.h)."""

    _fields_ = [("energy_ms", C.c_double), ("chroma_ms", C.c_double), ("novelty_ms", C.c_double), ("cells", u64)]


class SdspRequestSet(C.Structure):
    """sdsp_request_set: the optional requests of sdsp_analyze_batch_device_with, by name."""

    _fields_ = [
        ("struct_size", u32),
        ("ov_req", C.POINTER(SdspOverviewRequest)),
        ("overviews", C.POINTER(SdspOverview)),
        ("kt_req", C.POINTER(SdspKeyTimelineRequest)),
        ("timelines", C.POINTER(SdspKeyTimeline)),
        ("lv_req", C.POINTER(SdspLevelsRequest)),
        ("levels", C.POINTER(SdspLevels)),
        ("tm_req", C.POINTER(SdspTempoMapRequest)),
        ("tempo_maps", C.POINTER(SdspTempoMap)),
    ]


class SdspRequestSetExt(C.Structure):
    """sdsp_request_set_ext: sdsp_request_set, then the pairs added after the tempo map.  Pass
    byref(ext.base) with ext.base.struct_size = sizeof(ext)."""

    _fields_ = [
        ("base", SdspRequestSet),
        ("sc_req", C.POINTER(SdspSectionsRequest)),
        ("sections", C.POINTER(SdspSections)),
    ]


R128_LOUDNESS, R128_TRUE_PEAK, R128_CURVES = 1, 2, 4
R128_BITS = {"loudness": R128_LOUDNESS, "true-peak": R128_TRUE_PEAK, "curves": R128_CURVES}


class SdspR128Request(C.Structure):
    """sdsp_r128_request: a mask of sdsp_r128_what bits."""

    _fields_ = [("what", u32)]


class SdspR128(C.Structure):
    """sdsp_r128: one track's programme loudness (the two curves library-owned, one allocation)."""

    _fields_ = [
        ("status", C.c_int32),
        ("has_integrated", C.c_int8),
        ("has_range", C.c_int8),
        ("integrated_lufs", f32),
        ("range_lu", f32),
        ("range_low_lufs", f32),
        ("range_high_lufs", f32),
        ("max_momentary_lufs", f32),
        ("max_short_term_lufs", f32),
        ("sample_peak", f32),
        ("true_peak", f32),
        ("sample_peak_db", f32),
        ("true_peak_dbtp", f32),
        ("n_samples", u64),
        ("step_samples", u32),
        ("n_steps", u64),
        ("n_momentary", u64),
        ("n_short_term", u64),
        ("n_gated_momentary", u64),
        ("n_gated_short_term", u64),
        ("shelf", f32 * 5),
        ("highpass", f32 * 5),
        ("momentary", C.POINTER(f32)),
        ("short_term", C.POINTER(f32)),
    ]


class SdspRequestSetExt2(C.Structure):
    """sdsp_request_set_ext2: sdsp_request_set_ext, then the pair added after sections.  Pass
    byref(ext2.base.base) with ext2.base.base.struct_size = sizeof(ext2)."""

    _fields_ = [
        ("base", SdspRequestSetExt),
        ("r128_req", C.POINTER(SdspR128Request)),
        ("r128", C.POINTER(SdspR128)),
    ]


class SdspDebugR128Times(C.Structure):
    """sdsp_debug_r128_times (include/stratum_hip_debug.h)."""

    _fields_ = [("steps_ms", C.c_double), ("peak_ms", C.c_double), ("track_ms", C.c_double), ("tracks", u64),
                ("steps", u64)]


FP_WORDS, FP_MATCH = 1, 2
FP_BITS = {"words": FP_WORDS, "match": FP_MATCH}


class SdspFingerprintRequest(C.Structure):
    """sdsp_fingerprint_request."""

    _fields_ = [("what", u32), ("cell_seconds", f32), ("cell_samples", u64), ("max_offset_words", u32),
                ("min_overlap_words", u32), ("max_ber", f32)]


class SdspFingerprint(C.Structure):
    """sdsp_fingerprint: one track's fingerprint (the words library-owned)."""

    _fields_ = [("status", C.c_int32), ("n_cells", u64), ("n_words", u64), ("cell_samples", u64), ("first_sample", u64),
                ("n_matches", u64), ("words", C.POINTER(u32))]


class SdspFingerprintMatch(C.Structure):
    """sdsp_fingerprint_match."""

    _fields_ = [("a", u64), ("b", u64), ("offset_words", C.c_int32), ("offset_samples", C.c_int64), ("bit_errors", u64),
                ("bits_compared", u64), ("ber", f32)]


class SdspFingerprintMatches(C.Structure):
    """sdsp_fingerprint_matches: a call's match list (library-owned)."""

    _fields_ = [("n_compared", u64), ("n_pairs", u64), ("n_matches", u64), ("matches", C.POINTER(SdspFingerprintMatch))]


class SdspRequestSetExt3(C.Structure):
    """sdsp_request_set_ext3: sdsp_request_set_ext2, then the fingerprint request's fields.  Pass
    byref(ext3.base.base.base) with its struct_size = sizeof(ext3)."""

    _fields_ = [
        ("base", SdspRequestSetExt2),
        ("fp_req", C.POINTER(SdspFingerprintRequest)),
        ("fingerprints", C.POINTER(SdspFingerprint)),
        ("fp_matches", C.POINTER(SdspFingerprintMatches)),
    ]


class SdspDebugFingerprintOut(C.Structure):
    """sdsp_debug_fingerprint_out (include/stratum_hip_debug.h)."""

    _fields_ = [("cell_capacity", u64), ("word_capacity", u64), ("n_cells", C.POINTER(u64)), ("n_words", C.POINTER(u64)),
                ("m", C.POINTER(f32)), ("words", C.POINTER(u32))]


class SdspDebugFingerprintPair(C.Structure):
    """sdsp_debug_fingerprint_pair (include/stratum_hip_debug.h)."""

    _fields_ = [("offset_words", C.c_int32), ("eligible", u32), ("bit_errors", u32), ("positions", u32)]


class SdspDebugFingerprintTimes(C.Structure):
    """sdsp_debug_fingerprint_times (include/stratum_hip_debug.h)."""

    _fields_ = [("cells_ms", C.c_double), ("words_ms", C.c_double), ("match_ms", C.c_double), ("words", u64),
                ("compared", u64), ("pairs", u64)]


class SdspDebugLevelsTimes(C.Structure):
    """sdsp_debug_levels_times (include/stratum_hip_debug.h)."""

    _fields_ = [("fold_ms", C.c_double), ("fold2_ms", C.c_double), ("tracks", u64)]


OVERVIEW_ARRAYS = ("smin", "smax", "low", "mid", "high")


NOTE_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
FLAG_NAMES = ["MultimodalBpm", "WeakTonality", "TempoVariation", "OnsetDetectionAmbiguous"]
ERROR_NAMES = {1: "InvalidInput", 2: "DecodingError", 3: "ProcessingError", 4: "NotImplemented", 5: "NumericalError"}


def key_name(mode, tonic):
    """Key::name, result.rs:30-39."""
    return NOTE_NAMES[tonic % 12] + ("m" if mode == 1 else "")


def key_numerical(mode, tonic):
    """Key::numerical, result.rs:59-87."""
    maj = [0, 7, 2, 9, 4, 11, 6, 1, 8, 3, 10, 5]
    mnr = [9, 4, 11, 6, 1, 8, 3, 10, 5, 0, 7, 2]
    tab = maj if mode == 0 else mnr
    pos = tab.index(tonic % 12) if (tonic % 12) in tab else 0
    return f"{pos + 1}{'A' if mode == 0 else 'B'}"


def key_from_numerical(notation):
    """Key::from_numerical, result.rs:113-140 -> (mode, tonic) or None."""
    import re

    if len(notation.encode()) < 2:
        return None
    num_str, suffix = notation[:-1], notation[-1]
    if not re.fullmatch(r"\+?[0-9]+", num_str):  # u32::from_str
        return None
    num = int(num_str)
    if not 1 <= num <= 12:
        return None
    maj = [0, 7, 2, 9, 4, 11, 6, 1, 8, 3, 10, 5]
    mnr = [9, 4, 11, 6, 1, 8, 3, 10, 5, 0, 7, 2]
    if suffix == "A":
        return (0, maj[num - 1])
    if suffix == "B":
        return (1, mnr[num - 1])
    return None


def _tri(v):
    return None if v < 0 else bool(v)


def result_to_dict(r: SdspResult) -> dict:
    """AnalysisResult as a plain dict (serde field names, result.rs:186-263)."""
    beats = [r.beats[i] for i in range(r.n_beats)] if r.n_beats else []
    downs = [r.downbeats[i] for i in range(r.n_downbeats)] if r.n_downbeats else []
    bars = [r.bars[i] for i in range(r.n_bars)] if r.n_bars else []
    warns = [r.warnings[i].decode() for i in range(r.n_warnings)] if r.n_warnings else []
    flags = [FLAG_NAMES[i] for i in range(4) if r.flags & (1 << i)]
    d = {
        "bpm": r.bpm,
        "bpm_confidence": r.bpm_confidence,
        "key": {"Major" if r.key_mode == 0 else "Minor": r.key_tonic},
        "key_name": key_name(r.key_mode, r.key_tonic),
        "key_confidence": r.key_confidence,
        "key_clarity": r.key_clarity,
        "beat_grid": {"downbeats": downs, "beats": beats, "bars": bars},
        "grid_stability": r.grid_stability,
        "metadata": {
            "duration_seconds": r.duration_seconds,
            "sample_rate": r.sample_rate,
            "processing_time_ms": r.processing_time_ms,
            "algorithm_version": r.algorithm_version.decode(),
            "onset_method_consensus": r.onset_method_consensus,
            "methods_used": ["energy_flux", "chroma_extraction", "key_detection"],
            "flags": flags,
            "confidence_warnings": warns,
            "tempogram_multi_res_triggered": _tri(r.tempogram_multi_res_triggered),
            "tempogram_multi_res_used": _tri(r.tempogram_multi_res_used),
            "tempogram_percussive_triggered": _tri(r.tempogram_percussive_triggered),
            "tempogram_percussive_used": _tri(r.tempogram_percussive_used),
        },
    }
    if r.has_tempogram_candidates:
        d["metadata"]["tempogram_candidates"] = [
            {
                "bpm": r.tempogram_candidates[i].bpm,
                "score": r.tempogram_candidates[i].score,
                "fft_norm": r.tempogram_candidates[i].fft_norm,
                "autocorr_norm": r.tempogram_candidates[i].autocorr_norm,
                "selected": bool(r.tempogram_candidates[i].selected),
            }
            for i in range(r.n_tempogram_candidates)
        ]
    return d
