"""ctypes binding of libtbcheck.so (include/tbcheck.h, include/tbsynth.h).

This is the Python stand-in for the JNA binding a Clojure caller would use
(INTEGRATION.md): same entry points, same structs.  The library is built
in-tree by `build()` (hipcc, gfx950) and there is NO fallback: if the shared
object is missing or a GPU entry point reports TBC_ERR_NO_DEVICE the caller
gets an exception, never a CPU answer.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# TBC_LIB_PATH: load another build of the SAME library (A/B runs of kernel variants on the GPU box)
LIB_PATH = os.environ.get("TBC_LIB_PATH") or os.path.join(CSRC, "libtbcheck.so")

NIL = -(2 ** 31)
POS_CRASHED = 0xFFFFFFFF
NO_OP = 0xFFFFFFFF
MAX_FINAL_CONFIGS = 10

# :type
INVOKE, OK, FAIL, INFO = 0, 1, 2, 3
# :f
F_READ, F_WRITE, F_CAS, F_ACQUIRE, F_RELEASE, F_ADD, F_TXN, F_TRANSFER, F_CLASS = range(9)
# models
MODEL_REGISTER, MODEL_CAS_REGISTER, MODEL_MUTEX, MODEL_TABLE, MODEL_MULTI_REGISTER, MODEL_SET, MODEL_BANK = range(7)
# algorithms
ALG_COMPETITION, ALG_WGL, ALG_LINEAR = 0, 1, 2
# verdicts / causes
VALID, INVALID, UNKNOWN = 1, 0, -1
CAUSE_NONE, CAUSE_TIME_LIMIT, CAUSE_STEP_LIMIT, CAUSE_VISITED_FULL = 0, 1, 2, 3
DOM_NO_EAGER_READS, DOM_NO_TWIN_RULE, DOM_NO_COUNT_FORM, DOM_NO_LAZY_COMMUTING, DOM_STALL_HANDOVER, DOM_NO_ORDER_RESTARTS = 1, 2, 4, 8, 16, 32
DOM_NO_EAGER_TXNS, DOM_NO_TXN_INDEPENDENCE = 64, 128
# tbc_opts.list_order (16 + W: completion order, a :write as if it completed W ranks later; the default where it applies is 16 + 24)
ORDER_DEFAULT, ORDER_SLOT, ORDER_COMPLETION, ORDER_WRITES_LAST, ORDER_WRITE_DELAY = 0, 1, 2, 3, 16
# status
(OK_STATUS, ERR_INVALID_ARG, ERR_BAD_HISTORY, ERR_NO_DEVICE, ERR_OOM, ERR_WINDOW_TOO_WIDE,
 ERR_MODEL, ERR_HIP, ERR_UNSUPPORTED) = range(9)


class TbcError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__(f"libtbcheck status {status}: {detail}")
        self.status = status
        self.detail = detail


class NoDeviceError(TbcError):
    pass


class Events(C.Structure):
    _fields_ = [("n", C.c_uint32), ("type", C.POINTER(C.c_uint8)), ("process", C.POINTER(C.c_int32)),
                ("f", C.POINTER(C.c_uint8)), ("a", C.POINTER(C.c_int32)), ("b", C.POINTER(C.c_int32))]


class Ops(C.Structure):
    _fields_ = [("n", C.c_uint32), ("n_events", C.c_uint32), ("f", C.POINTER(C.c_uint8)),
                ("a", C.POINTER(C.c_int32)), ("b", C.POINTER(C.c_int32)), ("process", C.POINTER(C.c_int32)),
                ("inv_pos", C.POINTER(C.c_uint32)), ("ret_pos", C.POINTER(C.c_uint32)),
                ("pool", C.POINTER(C.c_int32)), ("pool_len", C.c_uint32), ("n_process", C.c_uint32)]


class Model(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("init", C.c_int32), ("table", C.POINTER(C.c_uint16)),
                ("n_states", C.c_uint32), ("n_classes", C.c_uint32), ("n_keys", C.c_uint32),
                ("flags", C.c_uint32)]


class Opts(C.Structure):
    _fields_ = [("algorithm", C.c_uint32), ("device", C.c_uint32), ("time_limit_ms", C.c_uint64),
                ("max_steps", C.c_uint64), ("max_visited_bytes", C.c_uint64),
                ("want_witness", C.c_uint32), ("visited_per_op", C.c_uint32),
                ("search_width", C.c_uint32), ("round_budget", C.c_uint32),
                ("lookahead", C.c_uint32), ("dominance", C.c_uint32), ("lanes_per_history", C.c_uint32), ("list_order", C.c_uint32)]


class Config(C.Structure):
    _fields_ = [("state", C.c_int32), ("last_op", C.c_uint32), ("n_pending", C.c_uint32),
                ("n_linearized", C.c_uint32), ("pending", C.c_uint32 * 16), ("linearized_mask", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("visited", C.c_uint64), ("probes", C.c_uint64),
                ("backtracks", C.c_uint64), ("max_depth", C.c_uint64), ("table_slots", C.c_uint64),
                ("ns_pack", C.c_uint64), ("ns_search", C.c_uint64), ("ns_total", C.c_uint64)]


class Result(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("analyzer", C.c_uint32),
                ("fail_op", C.c_uint32), ("prev_ok_op", C.c_uint32), ("final_state", C.c_int32),
                ("n_witness", C.c_uint32), ("search_width", C.c_uint32), ("witness", C.POINTER(C.c_uint32)), ("n_configs", C.c_uint32),
                ("configs", Config * MAX_FINAL_CONFIGS), ("counters", Counters)]


class BatchDesc(C.Structure):
    _fields_ = [("n_hist", C.c_uint32), ("op_off", C.POINTER(C.c_uint64)), ("n_events", C.POINTER(C.c_uint32)),
                ("n_process", C.POINTER(C.c_uint32)), ("cols", Ops), ("model_aux", C.POINTER(C.c_int32))]


class SweepInfo(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("seg_target", C.c_uint32), ("max_segs", C.c_uint32),
                ("cut_open", C.c_uint32), ("n_dom", C.c_uint32), ("n_segments", C.c_uint32), ("n_fallback", C.c_uint32)]


class SweepRel(C.Structure):
    """tbc_sweep_rel: what one wavefront of the level sweep hands on (exchanged between ranks as raw bytes)."""
    _fields_ = [("status", C.c_uint32), ("F0", C.c_uint32), ("F1", C.c_uint32), ("n_org", C.c_uint32),
                ("max_level", C.c_uint32), ("subrounds", C.c_uint32), ("n_end", C.c_uint32), ("end_state", C.c_uint32),
                ("configs_total", C.c_uint64), ("probes", C.c_uint64),
                ("M", (C.c_uint32 * 4) * 32), ("last_level", C.c_uint32 * 32)]


class SweepVerdict(C.Structure):
    _fields_ = [("valid", C.c_int32), ("fail_level", C.c_uint32), ("fail_seg", C.c_uint32), ("live_in", C.c_uint32 * 4),
                ("final_bits", C.c_uint32), ("end_state", C.c_uint32), ("n_wavefronts", C.c_uint32),
                ("probes", C.c_uint64), ("configs_total", C.c_uint64), ("subrounds", C.c_uint64), ("max_level", C.c_uint64)]


SWEEP_SLICES = 4


class SetFullIn(C.Structure):
    _fields_ = [("n_elements", C.c_uint32), ("n_reads", C.c_uint32), ("words_per_row", C.c_uint32), ("device", C.c_uint32),
                ("add_invoke", C.POINTER(C.c_uint32)), ("add_ok", C.POINTER(C.c_uint32)), ("read_invoke", C.POINTER(C.c_uint32)),
                ("read_ok", C.POINTER(C.c_uint32)), ("present", C.POINTER(C.c_uint32))]


class SetFullRows(C.Structure):
    _fields_ = [("n_elements", C.c_uint32), ("n_reads", C.c_uint32), ("device", C.c_uint32), ("reserved0", C.c_uint32),
                ("add_invoke", C.POINTER(C.c_uint32)), ("add_ok", C.POINTER(C.c_uint32)), ("read_invoke", C.POINTER(C.c_uint32)),
                ("read_ok", C.POINTER(C.c_uint32)), ("top", C.POINTER(C.c_uint32)), ("exc_off", C.POINTER(C.c_uint64)),
                ("exc", C.POINTER(C.c_uint32))]


class SetFullOut(C.Structure):
    _fields_ = [("known", C.POINTER(C.c_uint32)), ("last_present", C.POINTER(C.c_uint32)), ("last_absent", C.POINTER(C.c_uint32)),
                ("ns_scan", C.c_uint64), ("bytes_scanned", C.c_uint64), ("bytes_matrix", C.c_uint64)]


class SetFullKeysIn(C.Structure):
    _fields_ = [("n_keys", C.c_uint32), ("device", C.c_uint32), ("n_elements", C.POINTER(C.c_uint32)), ("n_reads", C.POINTER(C.c_uint32)),
                ("add_invoke", C.POINTER(C.c_uint32)), ("add_ok", C.POINTER(C.c_uint32)), ("read_invoke", C.POINTER(C.c_uint32)),
                ("read_ok", C.POINTER(C.c_uint32)), ("top", C.POINTER(C.c_uint32)), ("exc_off", C.POINTER(C.c_uint64)),
                ("exc", C.POINTER(C.c_uint32))]


class SetFullKeysOut(C.Structure):
    _fields_ = [("known", C.POINTER(C.c_uint32)), ("last_present", C.POINTER(C.c_uint32)), ("last_absent", C.POINTER(C.c_uint32)),
                ("ns_scan", C.c_uint64), ("bytes_scanned", C.c_uint64), ("bytes_matrix", C.c_uint64)]


SETFULL_F_LINEARIZABLE = 1
SETFULL_NEVER_READ, SETFULL_STABLE, SETFULL_LOST = 0, 1, 2
SETFULL_VALID_FALSE, SETFULL_VALID_TRUE, SETFULL_VALID_UNKNOWN = 0, 1, 2
SETFULL_WORST = 8


class SetFullTimes(C.Structure):
    _fields_ = [("op_time", C.POINTER(C.c_int64)), ("time_off", C.POINTER(C.c_uint64)), ("unit", C.c_uint64), ("flags", C.c_uint32),
                ("reserved0", C.c_uint32)]


class SetFullKeySummary(C.Structure):
    _fields_ = [("attempt_count", C.c_uint32), ("stable_count", C.c_uint32), ("lost_count", C.c_uint32), ("never_read_count", C.c_uint32),
                ("stale_count", C.c_uint32), ("valid", C.c_uint8), ("stable_q_present", C.c_uint8), ("lost_q_present", C.c_uint8),
                ("n_worst", C.c_uint8), ("stable_q", C.c_int64 * 5), ("lost_q", C.c_int64 * 5), ("worst_element", C.c_uint32 * SETFULL_WORST),
                ("worst_known", C.c_uint32 * SETFULL_WORST), ("worst_last_absent", C.c_uint32 * SETFULL_WORST),
                ("worst_latency", C.c_int64 * SETFULL_WORST)]


class SetFullResultsOut(C.Structure):
    _fields_ = [("outcome", C.POINTER(C.c_uint8)), ("stable_latency", C.POINTER(C.c_int64)), ("lost_latency", C.POINTER(C.c_int64)),
                ("known", C.POINTER(C.c_uint32)), ("last_present", C.POINTER(C.c_uint32)), ("last_absent", C.POINTER(C.c_uint32)),
                ("summary", C.POINTER(SetFullKeySummary)), ("ns_scan", C.c_uint64), ("ns_results", C.c_uint64), ("bytes_scanned", C.c_uint64),
                ("bytes_matrix", C.c_uint64)]


# tbc_setfull_keys_create_ops: the history as op columns (include/tbcheck.h TBC_SETFULL_T_* / TBC_SETFULL_OP_*)
SETFULL_T_INVOKE, SETFULL_T_OK, SETFULL_T_FAIL, SETFULL_T_INFO = 0, 1, 2, 3
SETFULL_T_NIL = 0x80
SETFULL_OP_OTHER, SETFULL_OP_ADD, SETFULL_OP_READ = 0, 1, 2
SETFULL_ENCODE_WINDOW_WORDS = 8192


class SetFullOpsIn(C.Structure):
    _fields_ = [("n_keys", C.c_uint32), ("device", C.c_uint32), ("op_off", C.POINTER(C.c_uint64)), ("index", C.POINTER(C.c_uint32)),
                ("type", C.POINTER(C.c_uint8)), ("f", C.POINTER(C.c_uint8)), ("process", C.POINTER(C.c_int64)),
                ("value", C.POINTER(C.c_int64)), ("val_off", C.POINTER(C.c_uint64)), ("vals", C.POINTER(C.c_int64))]


class SetFullEncoding(C.Structure):
    _fields_ = [("n_elements", C.POINTER(C.c_uint32)), ("n_reads", C.POINTER(C.c_uint32)), ("element", C.POINTER(C.c_int64)),
                ("add_invoke", C.POINTER(C.c_uint32)), ("add_ok", C.POINTER(C.c_uint32)), ("read_invoke", C.POINTER(C.c_uint32)),
                ("read_ok", C.POINTER(C.c_uint32)), ("dup_max", C.POINTER(C.c_uint32)), ("dup_count", C.POINTER(C.c_uint32)),
                ("unknown_values", C.POINTER(C.c_uint64)), ("ns_encode", C.c_uint64)]


# tbc_ledger_check: the ledger workload's checkers from op columns (include/tbcheck.h TBC_LEDGER_*)
LEDGER_T_INVOKE, LEDGER_T_OK, LEDGER_T_FAIL, LEDGER_T_INFO = 0, 1, 2, 3
LEDGER_K_OTHER, LEDGER_K_TRANSFER, LEDGER_K_READ, LEDGER_K_LOOKUP = 0, 1, 2, 3
LEDGER_F_FINAL = 1
LEDGER_M_NIL = 1
LEDGER_E_NONE, LEDGER_E_UNEXPECTED_KEY, LEDGER_E_NIL_BALANCE, LEDGER_E_WRONG_TOTAL, LEDGER_E_NEGATIVE_VALUE = range(5)
LEDGER_LOOKUP_WINDOW_WORDS = 8192


class LedgerIn(C.Structure):
    _fields_ = [("n_ops", C.c_uint32), ("device", C.c_uint32), ("index", C.POINTER(C.c_uint32)), ("type", C.POINTER(C.c_uint8)),
                ("kind", C.POINTER(C.c_uint8)), ("flags", C.POINTER(C.c_uint8)), ("mop_off", C.POINTER(C.c_uint64)),
                ("mop_id", C.POINTER(C.c_int64)), ("mop_a", C.POINTER(C.c_int64)), ("mop_b", C.POINTER(C.c_int64)),
                ("mop_c", C.POINTER(C.c_int64)), ("mop_flags", C.POINTER(C.c_uint8)), ("accounts", C.POINTER(C.c_int64)),
                ("n_accounts", C.c_uint32), ("negative_balances", C.c_uint32), ("total_amount", C.c_int64)]


class LedgerErrors(C.Structure):
    _fields_ = [("count", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("worst", C.c_uint32)]


class LedgerSummary(C.Structure):
    _fields_ = [("read_count", C.c_uint32), ("error_count", C.c_uint32), ("first_error", C.c_uint32), ("lowest", C.c_uint32),
                ("highest", C.c_uint32), ("n_transfers", C.c_uint32), ("errors", LedgerErrors * 5), ("n_final_reads", C.c_uint32),
                ("final_reads_unlike", C.c_uint32), ("n_final_lookups", C.c_uint32), ("final_lookups_unlike", C.c_uint32),
                ("suspect_lookups", C.c_uint32), ("valid_si", C.c_uint8), ("valid_lookups", C.c_uint8), ("valid_final_reads", C.c_uint8),
                ("reserved0", C.c_uint8), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


class LedgerOut(C.Structure):
    _fields_ = [("read_error", C.POINTER(C.c_uint8)), ("read_total", C.POINTER(C.c_int64)), ("read_badness", C.POINTER(C.c_int64)),
                ("lookup_missing", C.POINTER(C.c_uint32)), ("final_read_unlike", C.POINTER(C.c_uint8)),
                ("final_lookup_unlike", C.POINTER(C.c_uint8)), ("summary", LedgerSummary)]


# tbc_ledger_realtime: realtime bounds on the posted counters of the ledger's reads (include/tbcheck.h)
LEDGER_RT_STALE, LEDGER_RT_FUTURE, LEDGER_RT_REGRESSED = 0, 1, 2


class LedgerRtIn(C.Structure):
    _fields_ = [("ledger", LedgerIn), ("process", C.POINTER(C.c_int32)), ("init_credits", C.POINTER(C.c_int64)),
                ("init_debits", C.POINTER(C.c_int64)), ("ok_transfers_apply", C.c_uint32), ("reserved0", C.c_uint32)]


class LedgerRtSummary(C.Structure):
    _fields_ = [("read_count", C.c_uint32), ("error_count", C.c_uint32), ("first_error", C.c_uint32), ("valid", C.c_uint32),
                ("errors", LedgerErrors * 3), ("n_definite", C.c_uint32), ("n_possible", C.c_uint32), ("foreign_sides", C.c_uint32),
                ("bad_amounts", C.c_uint32), ("n_checked", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


class LedgerRtOut(C.Structure):
    _fields_ = [("rt_bits", C.POINTER(C.c_uint8)), ("rt_miss", C.POINTER(C.c_int64)), ("mop_lo", C.POINTER(C.c_int64)),
                ("mop_hi", C.POINTER(C.c_int64)), ("mop_floor", C.POINTER(C.c_int64)), ("summary", LedgerRtSummary)]


# tbc_ledger_snapshots: the reads of a ledger as snapshots in one order (include/tbcheck.h); its input is a plain LedgerIn
LEDGER_SNAP_PARTIAL, LEDGER_SNAP_SKEWED = 1, 2


class LedgerSnapSummary(C.Structure):
    _fields_ = [("read_count", C.c_uint32), ("n_partial", C.c_uint32), ("valid", C.c_uint32), ("bad_values", C.c_uint32),
                ("skewed", LedgerErrors), ("n_candidates", C.c_uint32), ("reserved0", C.c_uint32), ("n_checked", C.c_uint64),
                ("n_pairs", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


class LedgerSnapOut(C.Structure):
    _fields_ = [("skew_count", C.POINTER(C.c_uint32)), ("skew_first", C.POINTER(C.c_uint32)), ("skew_key", C.POINTER(C.c_uint32)),
                ("snap_flags", C.POINTER(C.c_uint8)), ("summary", LedgerSnapSummary)]


# tbc_ledger_cycles: the cycle search over monotonic-key and realtime edges of a ledger's reads, partial reads included
# (include/tbcheck.h); its input is a LedgerRtIn
LEDGER_CYC_PARTIAL, LEDGER_CYC_ON_CYCLE, LEDGER_CYC_CORE = 1, 2, 4
LEDGER_CYCLES_MAX_CORE = 16384


class LedgerCyclesSummary(C.Structure):
    _fields_ = [("read_count", C.c_uint32), ("n_partial", C.c_uint32), ("n_core", C.c_uint32), ("valid", C.c_uint32),
                ("n_on_cycle", C.c_uint32), ("n_components", C.c_uint32), ("first", C.c_uint32), ("largest", C.c_uint32),
                ("largest_size", C.c_uint32), ("closure_rounds", C.c_uint32), ("bad_values", C.c_uint32), ("reserved0", C.c_uint32),
                ("n_checked", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


class LedgerCyclesOut(C.Structure):
    _fields_ = [("scc", C.POINTER(C.c_uint32)), ("cyc_flags", C.POINTER(C.c_uint8)), ("summary", LedgerCyclesSummary)]


# tbc_ledger_journal: the lookups of a ledger audited against the transfers, real time and the reads (include/tbcheck.h); its input is
# a LedgerRtIn
(LEDGER_JN_UNKNOWN, LEDGER_JN_ALTERED, LEDGER_JN_REPEATED, LEDGER_JN_FAILED, LEDGER_JN_EARLY, LEDGER_JN_LOST, LEDGER_JN_VANISHED,
 LEDGER_JN_AHEAD, LEDGER_JN_BEHIND, LEDGER_JN_KINDS) = range(10)
LEDGER_JN_ENTRY_UNKNOWN, LEDGER_JN_ENTRY_ALTERED = 1, 2
LEDGER_JN_XFER_REINVOKED, LEDGER_JN_XFER_NIL = 1, 2
LEDGER_JN_READ_AHEAD, LEDGER_JN_READ_BEHIND = 1, 2


class LedgerJournalSummary(C.Structure):
    _fields_ = [("n_lookups", C.c_uint32), ("n_xfer_mops", C.c_uint32), ("n_records", C.c_uint32), ("n_reinvoked", C.c_uint32),
                ("foreign_sides", C.c_uint32), ("bad_amounts", C.c_uint32), ("read_count", C.c_uint32), ("valid", C.c_uint32),
                ("errors", LedgerErrors * LEDGER_JN_KINDS), ("totals", C.c_uint64 * LEDGER_JN_KINDS), ("n_entries", C.c_uint64),
                ("n_checked", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


class LedgerJournalOut(C.Structure):
    _fields_ = [("entry_bits", C.POINTER(C.c_uint8)), ("lk_counts", C.POINTER(C.c_uint32)), ("lk_present", C.POINTER(C.c_uint32)),
                ("lk_vector", C.POINTER(C.c_int64)), ("rd_bits", C.POINTER(C.c_uint8)), ("rd_first", C.POINTER(C.c_uint32)),
                ("xfer_present", C.POINTER(C.c_uint32)), ("xfer_early", C.POINTER(C.c_uint32)), ("xfer_lost", C.POINTER(C.c_uint32)),
                ("xfer_vanished", C.POINTER(C.c_uint32)), ("xfer_flags", C.POINTER(C.c_uint8)), ("summary", LedgerJournalSummary)]


# tbc_perf_series: the series behind the reference's perf plots from op columns (include/tbcheck.h TBC_PERF_*)
PERF_T_INVOKE, PERF_T_OK, PERF_T_FAIL, PERF_T_INFO = 0, 1, 2, 3
PERF_O_NONE = 0
PERF_F_CLIENT = 1
PERF_SELECT_TILE = 2048


class PerfIn(C.Structure):
    _fields_ = [("n_ops", C.c_uint32), ("device", C.c_uint32), ("time", C.POINTER(C.c_int64)), ("process", C.POINTER(C.c_int32)),
                ("type", C.POINTER(C.c_uint8)), ("flags", C.POINTER(C.c_uint8)), ("f", C.POINTER(C.c_uint16)), ("n_f", C.c_uint32),
                ("reserved0", C.c_uint32)]


class PerfSizes(C.Structure):
    _fields_ = [("n_ops", C.c_uint32), ("n_f", C.c_uint32), ("nb_all", C.c_uint32), ("n_plot", C.c_uint32), ("t_max", C.c_int64)]


class PerfSummary(C.Structure):
    _fields_ = [("n_ops", C.c_uint32), ("n_client", C.c_uint32), ("n_invocations", C.c_uint32), ("n_matched", C.c_uint32),
                ("n_completions", C.c_uint32), ("n_f", C.c_uint32), ("nb_all", C.c_uint32), ("n_plot", C.c_uint32),
                ("max_cell", C.c_uint32), ("reserved0", C.c_uint32), ("t_max", C.c_int64), ("ns_device", C.c_uint64),
                ("bytes_in", C.c_uint64)]


class PerfOut(C.Structure):
    _fields_ = [("op_latency", C.POINTER(C.c_int64)), ("op_outcome", C.POINTER(C.c_uint8)), ("op_open_after", C.POINTER(C.c_int32)),
                ("q_count", C.POINTER(C.c_uint32)), ("q_value", C.POINTER(C.c_int64)), ("rate_count", C.POINTER(C.c_uint32)),
                ("open_last", C.POINTER(C.c_int32)), ("open_fill", C.POINTER(C.c_int32)), ("summary", PerfSummary)]


# tbc_pair_events_batch: tbc_pair_events for many histories a call, on the device (include/tbcheck.h)
PAIR_MAX_PROCESS = 4096
PAIR_NO_ROW = 0xFFFFFFFF


class EventBatch(C.Structure):
    _fields_ = [("n_hist", C.c_uint32), ("device", C.c_uint32), ("ev_off", C.POINTER(C.c_uint64)), ("type", C.POINTER(C.c_uint8)),
                ("process", C.POINTER(C.c_int32)), ("f", C.POINTER(C.c_uint8)), ("a", C.POINTER(C.c_int32)), ("b", C.POINTER(C.c_int32))]


class PairOut(C.Structure):
    _fields_ = [("ops_cap", C.c_uint64), ("op_off", C.POINTER(C.c_uint64)), ("n_events", C.POINTER(C.c_uint32)),
                ("n_process", C.POINTER(C.c_uint32)), ("f", C.POINTER(C.c_uint8)), ("a", C.POINTER(C.c_int32)), ("b", C.POINTER(C.c_int32)),
                ("process", C.POINTER(C.c_int32)), ("inv_pos", C.POINTER(C.c_uint32)), ("ret_pos", C.POINTER(C.c_uint32)),
                ("word", C.POINTER(C.c_uint32)), ("status", C.POINTER(C.c_int32)), ("bad_row", C.POINTER(C.c_uint32)),
                ("n_bad", C.c_uint32), ("reserved0", C.c_uint32), ("n_ops", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


# the packed event word (include/tbcheck.h TBC_EVENT_WORD): type bits 0-2, f bits 3-7, a bits 8-16, b bits 17-25
EVW_TYPE_UNKNOWN, EVW_F_ABOVE, EVW_NIL, EVW_UNFIT = 7, 16, 255, 256


class PackedEventBatch(C.Structure):
    _fields_ = [("n_hist", C.c_uint32), ("device", C.c_uint32), ("ev_off", C.POINTER(C.c_uint64)), ("ev_word", C.POINTER(C.c_uint32)),
                ("process", C.POINTER(C.c_int32))]


class BatchEvents(C.Structure):
    """tbc_batch_events: pointers into one pinned event slot of a batch (tbc_batch_map_events)."""
    _fields_ = [("n_hist_cap", C.c_uint32), ("reserved0", C.c_uint32), ("events_cap", C.c_uint64), ("ev_off", C.POINTER(C.c_uint64)),
                ("ev_word", C.POINTER(C.c_uint32)), ("process", C.POINTER(C.c_int32))]


class EventsReport(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("bad_row", C.POINTER(C.c_uint32)), ("n_bad", C.c_uint32), ("reserved0", C.c_uint32),
                ("n_ops", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64)]


class KeyedEvents(C.Structure):
    """tbc_keyed_events: ONE event history beside a key column (tbc_pair_keyed_events); ev_word set: the packed form"""
    _fields_ = [("n", C.c_uint32), ("device", C.c_uint32), ("key", C.POINTER(C.c_int32)), ("ev_word", C.POINTER(C.c_uint32)),
                ("process", C.POINTER(C.c_int32)), ("type", C.POINTER(C.c_uint8)), ("f", C.POINTER(C.c_uint8)), ("a", C.POINTER(C.c_int32)),
                ("b", C.POINTER(C.c_int32))]


class SplitOut(C.Structure):
    _fields_ = [("keys_cap", C.c_uint32), ("n_keys", C.c_uint32), ("keys", C.POINTER(C.c_int32)), ("ev_off", C.POINTER(C.c_uint64)),
                ("row_of", C.POINTER(C.c_uint32))]


class BatchKeyedEvents(C.Structure):
    """tbc_batch_keyed_events: pointers into one pinned event slot of a batch (tbc_batch_map_keyed_events)."""
    _fields_ = [("n_hist_cap", C.c_uint32), ("reserved0", C.c_uint32), ("events_cap", C.c_uint64), ("key", C.POINTER(C.c_int32)),
                ("ev_word", C.POINTER(C.c_uint32)), ("process", C.POINTER(C.c_int32))]


class KeyedReport(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("bad_row", C.POINTER(C.c_uint32)), ("n_bad", C.c_uint32), ("reserved0", C.c_uint32),
                ("n_ops", C.c_uint64), ("ns_device", C.c_uint64), ("bytes_in", C.c_uint64), ("n_keys", C.c_uint32), ("reserved1", C.c_uint32),
                ("keys", C.POINTER(C.c_int32)), ("row_of", C.POINTER(C.c_uint32))]


def events_desc_bytes(n_hist):
    """TBC_EVENTS_DESC_BYTES: what tbc_batch_submit_events brings back from the device"""
    return 16 + 8 * (n_hist + 1) + 16 * n_hist


class BatchInput(C.Structure):
    """tbc_batch_input: pointers into one pinned slot of a batch (tbc_batch_map_input)."""
    _fields_ = [("n_hist_cap", C.c_uint32), ("reserved0", C.c_uint32), ("ops_cap", C.c_uint64),
                ("op_off", C.POINTER(C.c_uint64)), ("n_events", C.POINTER(C.c_uint32)), ("n_process", C.POINTER(C.c_uint32)),
                ("word", C.POINTER(C.c_uint32)), ("inv_pos", C.POINTER(C.c_uint32)), ("ret_pos", C.POINTER(C.c_uint32))]


class Progress(C.Structure):
    """tbc_progress: a run that is out, seen from another thread (include/tbcheck.h tbc_batch_progress)."""
    _fields_ = [("n_histories", C.c_uint32), ("n_decided", C.c_uint32), ("phase", C.c_uint32), ("running", C.c_uint32), ("elapsed_ns", C.c_uint64)]


PHASE_IDLE, PHASE_PACK, PHASE_RETRIES = 0, 1, 2


class InputInfo(C.Structure):
    _fields_ = [("n_hist", C.c_uint32), ("pending", C.c_uint32), ("total_ops", C.c_uint64), ("bytes_copied", C.c_uint64),
                ("ns_copy", C.c_uint64), ("inputs_consumed", C.c_uint64), ("lists_regrown", C.c_uint32), ("n_hist_cap", C.c_uint32),
                ("ops_cap", C.c_uint64)]


WIRE_NIL = 0xFF


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_ops", C.c_uint32), ("n_procs", C.c_uint32), ("n_values", C.c_uint32),
                ("busy_permille", C.c_uint32), ("info_permille", C.c_uint32), ("read_permille", C.c_uint32),
                ("write_permille", C.c_uint32), ("corrupt_permille", C.c_uint32)]


STEP_FN = C.CFUNCTYPE(C.c_int64, C.c_int64, C.c_uint32, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)      # tbc_allgather_fn(user, send, recv, bytes)
COMM_ID_BYTES = 128

# every symbol the headers declare: (name, restype, argtypes)
SYMBOLS = {
    "tbc_pair_events": (C.c_int, [C.POINTER(Events), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tbc_pair_events_batch": (C.c_int, [C.POINTER(EventBatch), C.POINTER(PairOut)]),
    "tbc_pack_events": (C.c_int, [C.POINTER(Events), C.POINTER(C.c_uint32)]),
    "tbc_pair_packed_batch": (C.c_int, [C.POINTER(PackedEventBatch), C.POINTER(PairOut)]),
    "tbc_pair_keyed_events": (C.c_int, [C.POINTER(KeyedEvents), C.POINTER(SplitOut), C.POINTER(PairOut)]),
    "tbc_batch_map_keyed_events": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(BatchKeyedEvents)]),
    "tbc_batch_submit_keyed_events": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(KeyedReport)]),
    "tbc_batch_map_events": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(BatchEvents)]),
    "tbc_batch_submit_events": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(EventsReport)]),
    "tbc_check": (C.c_int, [C.POINTER(Ops), C.POINTER(Model), C.POINTER(Opts), C.POINTER(Result)]),
    "tbc_result_free": (None, [C.POINTER(Result)]),
    "tbc_batch_create": (C.c_int, [C.POINTER(BatchDesc), C.POINTER(Model), C.POINTER(Opts), C.POINTER(C.c_void_p)]),
    "tbc_batch_run": (C.c_int, [C.c_void_p, C.POINTER(Result)]),
    "tbc_batch_last_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "tbc_batch_last_turn_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "tbc_batch_last_counters": (C.c_int, [C.c_void_p, C.POINTER(Counters)]),
    "tbc_batch_device_bytes": (C.c_uint64, [C.c_void_p]),
    "tbc_batch_search_width": (C.c_uint32, [C.c_void_p]),
    "tbc_batch_lanes_per_history": (C.c_uint32, [C.c_void_p]),
    "tbc_batch_list_order": (C.c_uint32, [C.c_void_p]),
    "tbc_batch_last_raced": (C.c_uint32, [C.c_void_p]),
    "tbc_batch_sweep_info": (C.c_int, [C.c_void_p, C.POINTER(SweepInfo)]),
    "tbc_sweep_compose": (C.c_int, [C.POINTER(SweepRel), C.c_uint32, C.c_uint32, C.POINTER(SweepVerdict)]),
    "tbc_batch_set_shard": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "tbc_batch_sweep_partial": (C.c_int, [C.c_void_p]),
    "tbc_batch_sweep_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "tbc_batch_sweep_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Result)]),
    "tbc_batch_sweep_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(Result)]),
    "tbc_setfull_create": (C.c_int, [C.POINTER(SetFullIn), C.POINTER(C.c_void_p)]),
    "tbc_setfull_create_rows": (C.c_int, [C.POINTER(SetFullRows), C.POINTER(C.c_void_p)]),
    "tbc_setfull_run": (C.c_int, [C.c_void_p, C.POINTER(SetFullOut)]),
    "tbc_setfull_destroy": (None, [C.c_void_p]),
    "tbc_setfull_keys_create": (C.c_int, [C.POINTER(SetFullKeysIn), C.POINTER(C.c_void_p)]),
    "tbc_setfull_keys_run": (C.c_int, [C.c_void_p, C.POINTER(SetFullKeysOut)]),
    "tbc_setfull_keys_destroy": (None, [C.c_void_p]),
    "tbc_setfull_results": (C.c_int, [C.c_void_p, C.POINTER(SetFullTimes), C.POINTER(SetFullResultsOut)]),
    "tbc_setfull_keys_results": (C.c_int, [C.c_void_p, C.POINTER(SetFullTimes), C.POINTER(SetFullResultsOut)]),
    "tbc_setfull_keys_create_ops": (C.c_int, [C.POINTER(SetFullOpsIn), C.POINTER(C.c_void_p)]),
    "tbc_setfull_keys_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tbc_setfull_keys_encoding": (C.c_int, [C.c_void_p, C.POINTER(SetFullEncoding)]),
    "tbc_ledger_check": (C.c_int, [C.POINTER(LedgerIn), C.POINTER(LedgerOut)]),
    "tbc_ledger_realtime": (C.c_int, [C.POINTER(LedgerRtIn), C.POINTER(LedgerRtOut)]),
    "tbc_ledger_snapshots": (C.c_int, [C.POINTER(LedgerIn), C.POINTER(LedgerSnapOut)]),
    "tbc_ledger_journal": (C.c_int, [C.POINTER(LedgerRtIn), C.POINTER(LedgerJournalOut)]),
    "tbc_ledger_cycles": (C.c_int, [C.POINTER(LedgerRtIn), C.POINTER(LedgerCyclesOut)]),
    "tbc_perf_plan_sizes": (C.c_int, [C.POINTER(PerfIn), C.POINTER(PerfSizes)]),
    "tbc_perf_series": (C.c_int, [C.POINTER(PerfIn), C.POINTER(PerfOut)]),
    "tbc_batch_destroy": (None, [C.c_void_p]),
    "tbc_comm_unique_id": (C.c_int, [C.c_void_p]),
    "tbc_comm_init": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "tbc_comm_init_host": (C.c_int, [C.c_uint32, C.c_uint32, ALLGATHER_FN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "tbc_comm_rank": (C.c_uint32, [C.c_void_p]),
    "tbc_comm_world": (C.c_uint32, [C.c_void_p]),
    "tbc_comm_destroy": (None, [C.c_void_p]),
    "tbc_batch_sweep_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Result)]),
    "tbc_batch_map_input": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(BatchInput)]),
    "tbc_batch_submit_input": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "tbc_batch_reload": (C.c_int, [C.c_void_p, C.POINTER(BatchDesc)]),
    "tbc_batch_input_info": (C.c_int, [C.c_void_p, C.POINTER(InputInfo)]),
    "tbc_batch_progress": (C.c_int, [C.c_void_p, C.POINTER(Progress)]),
    "tbc_memo_build": (C.c_int, [C.c_int64, C.c_uint32, STEP_FN, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint16),
                                 C.POINTER(C.c_int64), C.POINTER(C.c_uint32)]),
    "tbc_version": (C.c_uint32, []),
    "tbc_strerror": (C.c_char_p, [C.c_int]),
    "tbc_last_error": (C.c_char_p, []),
    "tbc_device_count": (C.c_int32, []),
    "tbc_debug_peek": (C.c_int, [C.POINTER(C.c_uint32), C.c_uint32]),
    "tbs_gen_register": (C.c_int, [C.POINTER(SynthParams), C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint32)]),
}

_LIB = None
ABI_VERSION = 2          # include/tbcheck.h TBC_ABI_VERSION


def build(force: bool = False) -> str:
    """Compile libtbcheck.so for gfx950 with hipcc (in-tree, so it travels to the GPU box)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(_HERE, "..", "include", f) for f in ("tbcheck.h", "tbsynth.h")]
    stale = force or not os.path.exists(LIB_PATH) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8", "libtbcheck.so"])
    return LIB_PATH


def lib():
    """The loaded library; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc). There is no CPU fallback.")
        try:  # share torch's HIP runtime (same SONAME) when torch is in the process
            import torch  # noqa: F401
        except Exception:  # pragma: no cover
            pass
        _LIB = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(_LIB, name)
            fn.restype = res
            fn.argtypes = args
        if _LIB.tbc_version() != ABI_VERSION:      # the structs above are this version's: another layout would be read past its end
            v, _LIB = _LIB.tbc_version(), None
            raise ImportError(f"{LIB_PATH} has ABI version {v}, this binding is written for {ABI_VERSION}: rebuild (__graft_entry__.build())")
    return _LIB


def check_status(status: int):
    if status == OK_STATUS:
        return
    detail = lib().tbc_last_error().decode() or lib().tbc_strerror(status).decode()
    if status == ERR_NO_DEVICE:
        raise NoDeviceError(status, detail)
    raise TbcError(status, detail)
