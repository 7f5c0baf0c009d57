"""MI355X-native CTC forced-alignment hot path — drop-in for kokoro_align.align.

Public surface mirrors the reference (kokoro_align/align.py):
    ctc_best_path(log_probs, labels, beam_size=1000, max_move=4)   align.py:43
    best_path(input_file, voca_file, output_file)                  align.py:112
    align(best_path_file, mfcc_file, voca_file, align_file, remove_wordsep)   align.py:127
    pandas_read_align(files)                                       align.py:172
plus batched / device-resident entry points (ctc_best_path_batch, ctc_best_path_device), the best path over a band the caller
gives (ctc_best_path_banded[_batch|_device], diagonal_band, anchored_band, band_around_path, band_edge_contact) or that steers
itself by the scores and returns the table it walked (ctc_best_path_tracking[_batch|_device]), or started from a score row,
ended at a chosen cell and resumable from the row it returns (ctc_best_path_resume[_batch|_device], free_start_scores,
ctc_best_path_chunked), or both, so that the self-steering band crosses a cut (ctc_best_path_tracking_resume[_batch|_device],
ctc_best_path_tracking_chunked), with the number of frames of such a chunk that are final whatever follows
(ctc_best_path_determined[_batch|_device], ctc_best_path_tracking_determined[_batch|_device]) and the aligner built on it that
commits frames while it is fed (StreamingAligner), and the
forward-backward quality signal of a best path (ctc_path_posteriors[_batch|_device], segment_confidence), the label
occupancy of every frame (ctc_label_posteriors[_batch|_device], segment_agreement), the differentiable lattice
log-likelihood (lattice_log_likelihood) and the state posteriors at chosen frames behind the confidence of align()'s text
boundaries (ctc_state_posteriors[_batch|_device], boundary_frames, segment_boundary_confidence), and the expected duration of
every state with the expected frame of every boundary (ctc_state_durations[_batch|_device], phoneme_durations,
expected_crossing_frames, segment_boundary_shift), and whole alignments sampled from the posterior over the band's paths with
the spread of every boundary (ctc_sample_paths[_batch|_device], sampled_crossing_frames, segment_boundary_spread), and the
alignment with the most frames at the right state in expectation (ctc_mea_path[_batch|_device], path_outputs,
segment_path_disagreement), and the probability that the path passes through every phoneme at all, the soft form of the
reference's keep-or-drop test of a segment (ctc_state_visits[_batch|_device], phoneme_visits, phoneme_spans,
segment_expected_match), and the exact quantiles of every boundary's frame, the interval a cut lies in with a given probability
(ctc_boundary_quantiles[_batch|_device], boundary_cuts, segment_boundary_interval), and on the best-path side the per-frame
margin of a path over the best alignment that disagrees with it, from max-marginals in exact float64 max-plus arithmetic
(ctc_path_margins[_batch|_device], segment_boundary_margin, segment_min_margin); and the forward-backward itself resumable, a
chunk at a time from a caller-given start row to a caller-given end row (ctc_posteriors_resume[_batch|_device], free_end_scores,
ctc_label_posteriors_chunked, StreamingAligner(confidence=True)), and so are the margins, whose chunks return the uncut call's
bits (ctc_margins_resume[_batch|_device], ctc_path_margins_chunked, StreamingAligner(confidence="margin")), with rows of
max-marginals at chosen frames (ctc_state_margins).

The DP and backtrace run in the HIP C-ABI library (include/kokoro_align_amd.h); there is no
CPU fallback — importing works without a GPU, computing does not.
"""
from . import encoder, transcript  # noqa: F401
from .align import (  # noqa: F401
    StreamingAligner,
    align,
    anchored_band,
    band_around_path,
    band_edge_contact,
    best_path,
    ctc_best_path,
    ctc_best_path_banded,
    ctc_best_path_banded_batch,
    ctc_best_path_banded_device,
    ctc_best_path_batch,
    ctc_best_path_chunked,
    ctc_best_path_determined,
    ctc_best_path_determined_batch,
    ctc_best_path_determined_device,
    ctc_best_path_device,
    ctc_best_path_resume,
    ctc_best_path_resume_batch,
    ctc_best_path_resume_device,
    ctc_best_path_tracking,
    ctc_best_path_tracking_batch,
    ctc_best_path_tracking_chunked,
    ctc_best_path_tracking_determined,
    ctc_best_path_tracking_determined_batch,
    ctc_best_path_tracking_determined_device,
    ctc_best_path_tracking_device,
    ctc_best_path_tracking_resume,
    ctc_best_path_tracking_resume_batch,
    ctc_best_path_tracking_resume_device,
    diagonal_band,
    free_start_scores,
    log_softmax_device,
    pandas_read_align,
)
from .posteriors import (  # noqa: F401
    boundary_cuts,
    boundary_frames,
    ctc_boundary_quantiles,
    ctc_boundary_quantiles_batch,
    ctc_boundary_quantiles_device,
    ctc_label_posteriors,
    ctc_label_posteriors_batch,
    ctc_label_posteriors_device,
    ctc_mea_path,
    ctc_mea_path_batch,
    ctc_mea_path_device,
    ctc_path_margins,
    ctc_path_margins_batch,
    ctc_path_margins_device,
    ctc_path_margins_chunked,
    ctc_margins_resume,
    ctc_margins_resume_batch,
    ctc_margins_resume_device,
    ctc_state_margins,
    ctc_label_posteriors_chunked,
    ctc_path_posteriors,
    ctc_path_posteriors_batch,
    ctc_path_posteriors_device,
    ctc_posteriors_resume,
    ctc_posteriors_resume_batch,
    ctc_posteriors_resume_device,
    free_end_scores,
    ctc_sample_paths,
    ctc_sample_paths_batch,
    ctc_sample_paths_device,
    ctc_state_durations,
    ctc_state_durations_batch,
    ctc_state_durations_device,
    ctc_state_posteriors,
    ctc_state_posteriors_batch,
    ctc_state_posteriors_device,
    ctc_state_visits,
    ctc_state_visits_batch,
    ctc_state_visits_device,
    expected_crossing_frames,
    lattice_log_likelihood,
    path_outputs,
    phoneme_durations,
    phoneme_spans,
    phoneme_visits,
    sampled_crossing_frames,
    segment_agreement,
    segment_boundary_confidence,
    segment_boundary_interval,
    segment_boundary_margin,
    segment_boundary_shift,
    segment_boundary_spread,
    segment_confidence,
    segment_expected_match,
    segment_min_margin,
    segment_path_disagreement,
)
from ._lib import KAError, build_library, library_path, load_library  # noqa: F401

__version__ = "0.1.0"
