"""MI355X-native hybrid MPI + OpenMP + HIP sequence-alignment search framework.

Same capabilities as nmiz1987/MPI-OPENMP-CUDA (CLI ``./final``, stdin format, output lines), rebuilt
for gfx950: an O(L1*L2) diagonal-sweep HIP kernel, a chunked pinned-DMA pipeline per GPU, cost-balanced
decomposition over ranks, RCCL (torch.distributed "nccl") / MPI collectives and a node-shared input
window. See README.md and SURVEY.md.
"""
from .models.problem import Problem
from .models.scoring import PairClass, Semantics, Weights
from .ops.align import (PROFILE_DTYPE, RANK_COLS, SUMMARY_COLS, HipSearchEngine, TargetSet, align_hits_device,
                        align_profile_device, align_report_device, align_search, align_search_device,
                        align_summary_device, align_targets_device, align_targets_summary_device, align_topk_device,
                        align_targets_hits_device, align_targets_topk_device, align_targets_rank_device,
                        brute_force_native,
                        decode_keys, decode_wire_cpu, device_count, profile_offsets, report_scores, search_cpu,
                        search_hip, search_hits_cpu, search_keys_cpu, search_profile_cpu, search_report_cpu,
                        search_summary_cpu, search_targets_cpu, search_targets_summary_cpu, search_topk_cpu,
                        search_targets_hits_cpu, search_targets_topk_cpu, search_targets_rank_cpu,
                        targets_rank_catalog_rows, targets_rank_chunks,
                        summary_thresholds, summary_zscore, targets_best, targets_catalog_rows, targets_zscore,
                        wire_batch_of)
from .parallel.wire import WireSlice
from .utils.io import (format_hits, format_report, format_results, format_summary, format_targets,
                       format_targets_hits, format_targets_rank, format_targets_summary, format_targets_topk, format_topk,
                       write_results)
from .utils.synthetic import make_synthetic

__version__ = "0.1.0"
__all__ = [
    "Problem", "PairClass", "Semantics", "Weights", "HipSearchEngine", "align_search", "align_search_device",
    "brute_force_native", "device_count", "search_cpu", "search_hip", "format_results", "write_results",
    "make_synthetic", "search_keys_cpu", "decode_keys", "PROFILE_DTYPE", "profile_offsets", "search_profile_cpu",
    "search_topk_cpu", "align_profile_device", "align_topk_device", "format_topk",
    "search_report_cpu", "report_scores", "align_report_device", "format_report",
    "search_hits_cpu", "align_hits_device", "format_hits",
    "WireSlice", "decode_wire_cpu", "wire_batch_of",
    "SUMMARY_COLS", "search_summary_cpu", "align_summary_device", "summary_zscore", "summary_thresholds",
    "format_summary",
    "TargetSet", "search_targets_cpu", "align_targets_device", "targets_best", "targets_catalog_rows",
    "format_targets",
    "search_targets_summary_cpu", "align_targets_summary_device", "targets_zscore", "format_targets_summary",
    "search_targets_topk_cpu", "search_targets_hits_cpu", "align_targets_topk_device", "align_targets_hits_device",
    "format_targets_topk", "format_targets_hits",
    "RANK_COLS", "search_targets_rank_cpu", "align_targets_rank_device", "targets_rank_catalog_rows",
    "targets_rank_chunks", "format_targets_rank",
]
