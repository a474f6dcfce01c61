/*
 * tbcheck.h -- C-ABI of libtbcheck.so, the MI355X-native linearizability checker.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json's
 * north_star: the Wing-Gong/Lowe search behind
 *
 *     (knossos.wgl/analysis model history)
 *     (knossos.linear/analysis model history)
 *     (knossos.competition/analysis model history)
 *     (jepsen.checker/linearizable {:model m :algorithm a})
 *
 * None of those live in /root/reference: the reference reaches Knossos only
 * transitively through `jepsen "0.2.8-SNAPSHOT"` (project.clj:8) and never
 * calls the search.  There is therefore no existing
 * FFI to replace; every entry point below is a new design, and each one cites
 * the Clojure function (recalled from the public jepsen-io/knossos and
 * jepsen-io/jepsen libraries) or the reference call site whose work it takes
 * over.  The binding a maintainer would add (JNA) is in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns a tbc_status (0 = OK); no exception or abort ever
 *     crosses the boundary.
 *   - all entry points are re-entrant: jepsen.checker/compose and
 *     jepsen.independent/checker evaluate sub-checkers from several JVM threads
 *     (reference call sites: set_full.clj:155-158, tests/ledger.clj:363-367,
 *     core.clj:139-146), so a call owns its own HIP stream and arena.
 *   - there is NO CPU fallback in this library: without a usable gfx950 device
 *     every compute entry point returns TBC_ERR_NO_DEVICE.
 */
#ifndef TBCHECK_H
#define TBCHECK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: tbc_opts grew to 64 bytes (lanes_per_history, reserved0), tbc_batch_sweep_finish gained merged_bytes, tbc_opts.dominance
 * gained TBC_DOM_NO_COUNT_FORM.  A caller built against another version must refuse the library (tbc_version()).
 * Still 2, additive: the word that was reserved0 (must be 0) is tbc_opts.list_order, 0 = the library's choice; tbc_batch_list_order().
 * Still 2, additive (round 6): tbc_batch_map_input / _submit_input / _reload / _input_info (fresh histories into a batch's arenas),
 * tbc_comm_* (the sharded sweep's exchange behind the C-ABI); tbc_setfull_create_rows takes its exception lists in any order again.
 * Still 2, additive: tbc_ledger_snapshots and its structs.
 * Still 2, additive: tbc_ledger_journal and its structs.
 * Still 2, additive: tbc_ledger_cycles and its structs.
 * Still 2, additive: tbc_pair_events_batch and its structs.
 * Still 2, additive: tbc_pack_events, tbc_pair_packed_batch, tbc_batch_map_events / _submit_events and their structs.
 * Still 2, additive: tbc_pair_keyed_events, tbc_batch_map_keyed_events / _submit_keyed_events and their structs. */
#define TBC_ABI_VERSION 2u

/* ------------------------------------------------------------------ status */
typedef enum tbc_status {
  TBC_OK = 0,
  TBC_ERR_INVALID_ARG = 1,   /* null pointer, bad enum, inconsistent sizes      */
  TBC_ERR_BAD_HISTORY = 2,   /* unsorted invocations, return before invoke, ... */
  TBC_ERR_NO_DEVICE = 3,     /* no gfx950 device / HIP runtime failure          */
  TBC_ERR_OOM = 4,           /* host or device allocation failed                */
  TBC_ERR_WINDOW_TOO_WIDE = 5, /* more open processes than the kernels support  */
  TBC_ERR_MODEL = 6,         /* op not understood by the model / bad table      */
  TBC_ERR_HIP = 7,           /* a HIP call failed; see tbc_last_error()         */
  TBC_ERR_UNSUPPORTED = 8
} tbc_status;

/* ----------------------------------------------------------------- history
 *
 * Event level: one row per Jepsen history op map, exactly the columns the
 * reference's own checkers read -- :type :f :value :process (:index is the row
 * number).  Shapes: set_full.clj:29-31,42-45,113-116,128-134;
 * tests/ledger.clj:89-114; README.md:41-50,67-74.  Rows whose :process is not
 * an integer (:nemesis ...) must be dropped by the caller, as the reference
 * itself does with (int? process) at tests/ledger.clj:94,204,228.
 */
enum { TBC_INVOKE = 0, TBC_OK_ = 1, TBC_FAIL = 2, TBC_INFO = 3 };

/* op function codes (the :f of an op), shared by every model */
enum {
  TBC_F_READ = 0,     /* register family: a = value read or TBC_NIL             */
  TBC_F_WRITE = 1,    /* register family: a = value written                     */
  TBC_F_CAS = 2,      /* cas-register: a = expected, b = new                    */
  TBC_F_ACQUIRE = 3,  /* mutex                                                  */
  TBC_F_RELEASE = 4,  /* mutex                                                  */
  TBC_F_ADD = 5,      /* set: a = element                                       */
  TBC_F_TXN = 6,      /* multi-register: a = pool offset, b = #micro-ops        */
  TBC_F_TRANSFER = 7, /* bank: a = pool offset of {debit, credit, amount}       */
  TBC_F_CLASS = 8     /* table model: a = op class id (column of the table)     */
  /* TBC_F_READ on set/bank: a = pool offset, b = #values (or TBC_NIL in a)     */
};

#define TBC_NIL INT32_MIN             /* Clojure nil in a value column           */
#define TBC_POS_CRASHED 0xFFFFFFFFu   /* ret_pos of an op that never completed   */

typedef struct tbc_events {
  uint32_t n;               /* number of rows                                   */
  const uint8_t* type;      /* TBC_INVOKE / TBC_OK_ / TBC_FAIL / TBC_INFO       */
  const int32_t* process;   /* integer :process                                 */
  const uint8_t* f;         /* TBC_F_*                                          */
  const int32_t* a;         /* first value column                               */
  const int32_t* b;         /* second value column                              */
} tbc_events;

/*
 * Op level: the history after knossos.history/complete, /without-failures and
 * pairing (recalled: knossos.history complete, without-failures, pair-index;
 * reference uses of the same helpers: tests/ledger.clj:206,239,
 * checker/perf.clj:617,623).  One row per invocation that may have taken
 * effect, sorted by invocation position.  SoA, caller-owned, read-only.
 */
typedef struct tbc_ops {
  uint32_t n;               /* number of ops                                    */
  uint32_t n_events;        /* every position below is < n_events               */
  const uint8_t* f;         /* TBC_F_*                                          */
  const int32_t* a;         /* value column 0 (completed value for reads)       */
  const int32_t* b;         /* value column 1                                   */
  const int32_t* process;   /* dense process id, 0 <= process < n_process       */
  const uint32_t* inv_pos;  /* history position of the invocation, ascending    */
  const uint32_t* ret_pos;  /* position of the :ok completion, TBC_POS_CRASHED  */
  const int32_t* pool;      /* value pool for wide ops (may be NULL)            */
  uint32_t pool_len;
  uint32_t n_process;       /* number of distinct processes (= window slots)    */
} tbc_ops;

/*
 * tbc_pair_events: knossos.history/complete + without-failures + pairing.
 *   - an :ok completion's value columns replace its invocation's (a read learns
 *     what it read), a :fail completion deletes the pair, an :info completion
 *     or a missing one leaves the invocation open for ever (TBC_POS_CRASHED);
 *   - process ids are re-numbered densely in order of first appearance.
 * Output arrays are caller-allocated with capacity ev->n; *n_ops, *n_process
 * receive the counts.  ev_index[i] = row of op i's invocation (its :index).
 * Pure host code, no device needed: one history a call, one thread.  tbc_pair_events_batch (below, "pairing on the device") does
 * the same for many histories in one call on the device; this function is its specification.
 */
tbc_status tbc_pair_events(const tbc_events* ev,
                           uint8_t* f, int32_t* a, int32_t* b, int32_t* process,
                           uint32_t* inv_pos, uint32_t* ret_pos,
                           uint32_t* n_ops, uint32_t* n_process);

/* ------------------------------------------------------------------ models
 *
 * knossos.model constructors (recalled): register,
 * cas-register, mutex, multi-register, set.  Knossos ships no bank model; the
 * one here follows the reference's own ledger->bank mapping
 * (tests/ledger.clj:89-114; balance = credits - debits, :102-103).
 * TBC_MODEL_TABLE is knossos.model.memo/memo: a dense transition table
 * next = table[state * n_classes + class], 0xFFFF = inconsistent.
 *
 * Value pool (tbc_ops.pool, int32) layouts, written by the caller's encoder
 * (jepsen-tigerbeetle_amd/knossos/_analysis.py is the tested one):
 *   MULTI_REGISTER  :txn op: a = offset, b = #micro-ops of {f (0 read / 1 write),
 *                   key (0..n_keys-1, n_keys <= 8), value (0..13 or TBC_NIL for a
 *                   read)} triples.  State = 4 bits per key; tbc_model.init = packed
 *                   initial state (0 = all nil).
 *   SET             commutative, state-free.  tbc_model.init (or
 *                   tbc_batch_desc.model_aux[h]) = offset of nadds_before[0..R]
 *                   (R = number of :ok completions of the history, in row order).
 *                   :add op: a = index j of the add in completion order (crashed adds
 *                   last); :read op: a = TBC_NIL or offset of {nR, lead, bitset words}
 *                   (bitset over adds in j order; nR = |R| or -1 if R holds an element
 *                   nobody adds; lead = number of leading ones).  Elements unique.
 *   BANK            commutative (negative balances allowed), state-free.  n_keys =
 *                   #accounts (<= 16); init / model_aux = offset of
 *                   bal_before[(R+1) * n_keys]; :transfer a = offset of {debit index,
 *                   credit index, amount}; :read a = TBC_NIL or offset of the balances.
 * SET and BANK exist in the wide schedule only (search_width >= 2 is forced).
 */
enum {
  TBC_MODEL_REGISTER = 0,
  TBC_MODEL_CAS_REGISTER = 1,
  TBC_MODEL_MUTEX = 2,
  TBC_MODEL_TABLE = 3,
  TBC_MODEL_MULTI_REGISTER = 4,
  TBC_MODEL_SET = 5,
  TBC_MODEL_BANK = 6
};

#define TBC_TABLE_INCONSISTENT 0xFFFFu

typedef struct tbc_model {
  uint32_t kind;            /* TBC_MODEL_*                                      */
  int32_t init;             /* initial value (TBC_NIL for (cas-register))       */
  const uint16_t* table;    /* TBC_MODEL_TABLE only                             */
  uint32_t n_states;        /* TBC_MODEL_TABLE only                             */
  uint32_t n_classes;       /* TBC_MODEL_TABLE only                             */
  uint32_t n_keys;          /* multi-register keys / bank accounts              */
  uint32_t flags;           /* TBC_MODEL_F_*                                    */
} tbc_model;

enum { TBC_MODEL_F_NO_NEGATIVE = 1u }; /* bank: balances may not go negative    */

/* ----------------------------------------------------------------- options */
enum { TBC_ALG_COMPETITION = 0, TBC_ALG_WGL = 1, TBC_ALG_LINEAR = 2 };

typedef struct tbc_opts {
  uint32_t algorithm;        /* TBC_ALG_*; jepsen.checker/linearizable :algorithm */
  uint32_t device;           /* HIP device ordinal                               */
  uint64_t time_limit_ms;    /* 0 = none; exceeded => :valid? :unknown           */
  uint64_t max_steps;        /* 0 = none; search-step budget (deterministic)     */
  uint64_t max_visited_bytes;/* 0 = library default; visited-set cap per history */
  uint32_t want_witness;     /* copy the linearization order back                */
  uint32_t visited_per_op;   /* 0 = default (64): first visited-set capacity is   */
                             /* this many entries per op, x16 on each overflow    */
  uint32_t search_width;     /* configs expanded per iteration.  1 = the sequential*/
                             /* knossos.wgl order (witness and counters equal the */
                             /* published algorithm's); 2..16 = the wide schedule */
                             /* (same verdict / failing op, one (config, call)    */
                             /* pair per lane).  0 = default: 1 for TBC_ALG_WGL;  */
                             /* else 4, or 2 when the batch is a register /       */
                             /* cas-register one under the dominance rules with   */
                             /* at most 10 calls in flight on average (fewer      */
                             /* configs expanded in vain; tbc_batch_search_width) */
  uint32_t round_budget;     /* wide schedule, 0 = off: a history that has used     */
                             /* more rounds than this continues at search_width 16  */
                             /* (a batch's stragglers then need far fewer dependent */
                             /* rounds; the schedule stays deterministic)           */
  uint32_t lookahead;        /* wide schedule, register / cas-register: a new config  */
                             /* is SET ASIDE when one of the next 8 completions can   */
                             /* never be linearized from it (its call needs a value   */
                             /* that neither the state nor any call still to be       */
                             /* linearized provides); set-aside configs are expanded  */
                             /* only if the search would otherwise end invalid, so the*/
                             /* failing op and :configs stay exact.  0 = on, 1 = off  */
  uint32_t dominance;        /* wide schedule / level sweep, register / cas-register:  */
                             /* two rules that drop configs without changing a verdict */
                             /* or a failing op (TBC_DOM_*); 0 = both on               */
  uint32_t lanes_per_history;/* depth-first search, register / cas-register / mutex:    */
                             /* 4, 8, 16 or 32 = SEVERAL HISTORIES PER WAVEFRONT (64 / n  */
                             /* them, n lanes each; wgl_narrow.hip): one config per      */
                             /* iteration, n (config, call) pairs per round -- the       */
                             /* schedule for big batches at low concurrency, where a     */
                             /* round has few pairs.  64 = one history per wavefront     */
                             /* (search_width configs per round).  0 = the library       */
                             /* chooses: 8 for a batch of >= 24576 register-family       */
                             /* histories under both dominance rules with at most 10     */
                             /* calls in flight, if search_width is 0 too; else 64.      */
                             /* tbc_batch_lanes_per_history() says what was chosen.      */
  uint32_t list_order;       /* depth-first search, register / cas-register: the order   */
                             /* in which a config's open calls are tried (TBC_ORDER_*).   */
                             /* Verdict, failing op and :previous-ok do not depend on it; */
                             /* counters, witness and :configs are the chosen schedule's. */
                             /* 0 = the library chooses: in order of completion with a    */
                             /* :write as if it completed 24 ranks later (16 + 24) where  */
                             /* it applies (one mask word, no level sweep beside the      */
                             /* search, no count form, no round budget), else slot order. */
                             /* tbc_batch_list_order() says what a batch runs.            */
} tbc_opts;

/* tbc_opts.list_order.  The search takes a config's candidates last to first and pops the last child first, so the order of a
 * front's list of open calls decides which linearization is tried first.  SLOT: by process slot (rounds 1-4; what oracle/wgl_beam.c
 * runs unless told otherwise).  COMPLETION: the call that completes soonest first.  WRITES_LAST: ... and every :write after everything
 * else (a :cas the state allows now before a :write, which every state allows).  16 + W: in order of completion, a :write placed as
 * if it completed W ranks later (W <= 4096) -- the soft form; W = 24 halves the rounds at 19 calls in flight. */
enum { TBC_ORDER_DEFAULT = 0u, TBC_ORDER_SLOT = 1u, TBC_ORDER_COMPLETION = 2u, TBC_ORDER_WRITES_LAST = 3u, TBC_ORDER_WRITE_DELAY = 16u };

/* tbc_opts.dominance bits (set = rule OFF).  Eager reads: an open read whose value is nil or
 * the current state is linearized at once (it changes nothing, so every later schedule stays
 * possible); the search then branches over :write / :cas only.  Twin rule: of several open,
 * not yet linearized calls with the same effect the one completing first goes first.  Both
 * need register values in 0..30; a history outside that range is searched without them. */
enum { TBC_DOM_NO_EAGER_READS = 1u, TBC_DOM_NO_TWIN_RULE = 2u,
       /* COUNT FORM (knossos.competition on a register / cas-register history with crashed calls, both rules above on): crashed
        * calls of one effect are linearized in invocation order, so a config keeps a COUNT per effect class instead of a mask bit
        * per crashed call, process slots are re-used, a crashed call is only linearized right before a call that observes its
        * value, and a config that has used no fewer crashed calls of any class than a visited one with the same (front, mask,
        * state) is dropped.  A history the exact search does not decide within 32 probes per op OF THE BATCH'S LONGEST HISTORY (one
        * budget per launch) -- and only when the caller names no max_steps: a caller's own step limit is one exact pass under that
        * limit, nothing after it -- is first refuted with every
        * class an unlimited supply (a superset of the linearizations), then the prefix before the refuted completion is
        * linearized: verdict and failing op are exact, :configs of such a verdict holds the ONE config the prefix's linearization
        * ended in (the exact search's own exhaustion, when it names an earlier completion, reports its stuck configs as ever).
        * Set = keep one mask bit per crashed call (the published form). */
       TBC_DOM_NO_COUNT_FORM = 4u,
       /* LAZY RULE of the commutative models (set, bank): an :add / :transfer changes nothing a call other than a :read can see and
        * commutes with its kind, so without loss of generality it is linearized only when it completes at the front or when an open,
        * not yet linearized read could take it (set: a read whose value contains the element -- a crashed add no read ever contains
        * is never linearized; bank: a read with a value).  The config space is then no longer 2^(open or crashed mutating calls):
        * a 10k-op set history with 98 crashed adds needs 1.9 * 10^4 probes where the plain search gives up past 2 * 10^7.  Set = off. */
       TBC_DOM_NO_LAZY_COMMUTING = 8u,
       /* STALL HANDOVER -- the one bit of this word that switches something ON (a big quiet batch of register / cas-register histories,
        * several to a wavefront, nobody asking for a witness or naming a step limit): a history whose search has not passed a completion
        * for 4,096 rounds -- it is not linearizable, or in a burst of concurrency -- is stopped and checked again by the level sweep
        * (a few through tbc_check, many as a small batch).  For a batch that holds NOT LINEARIZABLE histories: 342 of 2,048 invalid, search
        * 159 -> 30 ms.  Off by default, measured: valid histories stall too (~10 of 32,768 bench histories at this threshold), they are
        * the ones with the biggest bursts, which the sweep is slowest at, and an all-valid batch pays 54 ms a pass for them while one bad
        * read in the middle of one history costs a pass 104 ms without the handover and 53 with it.  Verdict and failing op are the same
        * either way; the counters of a handed-over history are the stopped search's plus the sweep's, tbc_result.analyzer says who answered. */
       TBC_DOM_STALL_HANDOVER = 16u,
       /* ORDER RESTARTS (round 6; on by default where they apply: the wide depth-first search of a register / cas-register batch, one
        * history per wavefront, the library's own list order, no step limit named).  At high concurrency the cost of a depth-first
        * search is heavy-tailed in the ORDER its candidates are tried and nearly independent between orders (oracle counts, 24 histories
        * at ~32 calls in flight, seven orders: the default order's slowest > 2 * 10^6 probes, its median 192k; the best order per
        * history: slowest 341k, median 91k) -- and a pass over a batch is as long as its slowest history.  So the first pass runs under a
        * budget of 32 probes per op of the batch's longest history; a history that has not ended by then is searched AGAIN FROM SCRATCH
        * in other list orders (16 + 48, writes last, completion, 16 + 8, slot).  Nobody asking for a witness: in all six orders AT THE SAME
        * TIME, as small batches of their own on streams of their own -- the first search to decide a history stops the others' searches
        * of it (a race: knossos.competition's idea, between orders instead of algorithms); verdict and failing op are the search's in
        * any order, which order answers and hence the counters can differ from run to run.  With a witness: one order after the other
        * under the same budget, then the default order without one -- deterministic, the counters the sums over the passes, which
        * oracle/wgl.py check_restart_pipeline states pass by pass.  Set = one pass, no budget. */
       TBC_DOM_NO_ORDER_RESTARTS = 32u,
       /* multi-register (knossos.model/multi-register) under the wide schedule (search_width > 1), round 6; both on by default:
        * EAGER TXNS -- an open :txn of micro-reads only, each nil or what the state holds for its key, is linearized at once (it changes
        * nothing, so every later schedule stays possible; such calls are in the witness, not in the search's chain of branching calls).
        * TXN INDEPENDENCE -- txns conflict when one writes a key the other reads or writes, and txns that do not conflict commute.  At a
        * config whose front is the completion of call X, the candidates are the closure of {X} under "conflicts with" among the open calls
        * not yet linearized (persistent-set reduction: in any valid continuation the first member of that closure can be moved to the
        * front).  Same verdicts and failing ops; fewer configs (oracle/wgl_beam.c: 20k-op histories of 256 processes at 7.7 calls in
        * flight, > 3 * 10^7 probes plain, 4 - 7 * 10^6 under both). */
       TBC_DOM_NO_EAGER_TXNS = 64u, TBC_DOM_NO_TXN_INDEPENDENCE = 128u };

/* ------------------------------------------------------------------ result */
enum { TBC_VALID = 1, TBC_INVALID = 0, TBC_UNKNOWN = -1 };
enum {
  TBC_CAUSE_NONE = 0,
  TBC_CAUSE_TIME_LIMIT = 1,
  TBC_CAUSE_STEP_LIMIT = 2,
  TBC_CAUSE_VISITED_FULL = 3   /* visited set hit max_visited_bytes              */
};

#define TBC_MAX_FINAL_CONFIGS 10   /* jepsen.checker/linearizable truncates to 10 */
#define TBC_NO_OP 0xFFFFFFFFu

typedef struct tbc_config {      /* one knossos config: {:model :pending :last-op} */
  int32_t state;                 /* model state (value / table state id)          */
  uint32_t last_op;              /* op index linearized last, or TBC_NO_OP (always  */
                                 /* TBC_NO_OP from a several-histories-per-wavefront */
                                 /* batch that wants no witness: it keeps no links)  */
  uint32_t n_pending;            /* open ops at the front ...                     */
  uint32_t n_linearized;         /* ... of which this many are already linearized */
  uint32_t pending[16];          /* first 16 open op indices                      */
  uint32_t linearized_mask;      /* bit i: pending[i] is linearized               */
} tbc_config;

typedef struct tbc_counters {
  uint64_t steps;        /* candidate linearizations attempted (model step ok)   */
  uint64_t visited;      /* configs inserted into the visited set                */
  uint64_t probes;       /* visited-set lookups                                  */
  uint64_t backtracks;   /* frames popped                                        */
  uint64_t max_depth;    /* deepest DFS stack                                    */
  uint64_t table_slots;  /* final visited-set capacity (entries)                 */
  uint64_t ns_pack;      /* device time: history pack kernel                     */
  uint64_t ns_search;    /* device time: search kernel(s)                        */
  uint64_t ns_total;     /* wall time inside the call                            */
} tbc_counters;

typedef struct tbc_result {
  int32_t valid;             /* TBC_VALID / TBC_INVALID / TBC_UNKNOWN            */
  int32_t cause;             /* TBC_CAUSE_* when unknown                         */
  uint32_t analyzer;         /* TBC_ALG_WGL or TBC_ALG_LINEAR: who answered      */
  uint32_t fail_op;          /* invalid: op whose completion cannot be passed    */
  uint32_t prev_ok_op;       /* invalid: op completing just before it (:previous-ok) */
  int32_t final_state;       /* valid: model state after the witness             */
  uint32_t n_witness;        /* valid && want_witness: ops in `witness`, else 0  */
  uint32_t search_width;     /* configs per round of the depth-first search of   */
                             /* this call (what tbc_opts.search_width 0 became)  */
  uint32_t* witness;         /* valid && want_witness: op indices, library-owned */
  uint32_t n_configs;        /* final configs (<= TBC_MAX_FINAL_CONFIGS)         */
  tbc_config configs[TBC_MAX_FINAL_CONFIGS];
  tbc_counters counters;
} tbc_result;

/* --------------------------------------------------------- single history
 *
 * tbc_check == (knossos.wgl/analysis model history) et al.: host SoA in,
 * verdict out (H2D + pack kernel + search kernel + D2H).  `out` is caller
 * allocated; out->witness is library-allocated and released by
 * tbc_result_free.
 */
tbc_status tbc_check(const tbc_ops* ops, const tbc_model* model,
                     const tbc_opts* opts, tbc_result* out);
void tbc_result_free(tbc_result* r);

/* ------------------------------------------------------------- batch mode
 *
 * Many independent histories per launch -- what jepsen.independent/checker
 * does per key (set_full.clj:155) and BASELINE.json's batch configs ask for.
 * A batch owns device memory for its inputs, packed layout, stacks and
 * visited sets; inputs stay resident in HBM across tbc_batch_run calls.
 * Histories are concatenated: history h owns ops [op_off[h], op_off[h+1]).
 */
typedef struct tbc_batch tbc_batch;

typedef struct tbc_batch_desc {
  uint32_t n_hist;
  const uint64_t* op_off;     /* n_hist+1 offsets into the op columns            */
  const uint32_t* n_events;   /* per history                                     */
  const uint32_t* n_process;  /* per history                                     */
  tbc_ops cols;               /* concatenated columns; cols.n = total ops        */
  const int32_t* model_aux;   /* optional, per history: overrides tbc_model.init  */
                              /* (set / bank: pool offset of the history's own    */
                              /* per-front table when histories share one pool)   */
} tbc_batch_desc;

tbc_status tbc_batch_create(const tbc_batch_desc* desc, const tbc_model* model,
                            const tbc_opts* opts, tbc_batch** out);
/* one pass of the hot path over the resident batch: pack + search (+ retries
 * of histories whose visited set overflowed).  results: n_hist entries,
 * caller-allocated (witness pointers are library-owned, valid until the next
 * run or tbc_batch_destroy). */
tbc_status tbc_batch_run(tbc_batch* b, tbc_result* results);
/* device-time breakdown of the last run, ns, measured with HIP events on the
 * batch's own stream: [0] memset/init, [1] pack, [2] search, [3] retries */
tbc_status tbc_batch_last_timing(const tbc_batch* b, uint64_t ns[4]);
/* SEVERAL BATCHES IN FLIGHT.  A batch owns its stream and its arenas, so different batches may be run at the
 * same time from different host threads (tbc_batch_run holds no process-wide lock; one batch is still one
 * thread's at a time) -- which is how jepsen.independent/checker drives a checker: one (bounded-)pmap thread
 * per key group (the reference wraps its per-key checkers in jepsen.independent/checker at
 * src/tigerbeetle/workloads/set_full.clj:154-158).  Batches that run several histories per wavefront take the whole GPU for their search and the
 * library gives those searches the device one at a time, in launch order, through a device-side event; the
 * init and pack of the next batch run beside the search of the previous one (measured: 2 x 32,768 histories
 * in flight, 258k histories/s against 204k one batch after the other).  ns = how long the last run's search
 * waited for its turn (not counted in ns[2] of tbc_batch_last_timing). */
tbc_status tbc_batch_last_turn_wait(const tbc_batch* b, uint64_t* ns);
/* sum of tbc_counters over the last run (probes, visited ...) */
tbc_status tbc_batch_last_counters(const tbc_batch* b, tbc_counters* out);
uint64_t tbc_batch_device_bytes(const tbc_batch* b);
/* the search_width this batch runs the depth-first search at (what tbc_opts.search_width = 0 resolved to; 1 when
 * several histories share a wavefront) */
uint32_t tbc_batch_search_width(const tbc_batch* b);
/* lanes per history of the depth-first search: 4 / 8 / 16 / 32 (several histories per wavefront) or 64 */
uint32_t tbc_batch_lanes_per_history(const tbc_batch* b);
/* the order of the fronts' lists this batch's depth-first search runs over: TBC_ORDER_SLOT / _COMPLETION / _WRITES_LAST or 16 + W
 * (what tbc_opts.list_order = 0 resolved to; SLOT wherever another order does not apply) */
uint32_t tbc_batch_list_order(const tbc_batch* b);
/* histories of the last run whose first pass ended at its budget and that were then searched in several list orders at once
 * (tbc_opts.dominance, TBC_DOM_NO_ORDER_RESTARTS) */
uint32_t tbc_batch_last_raced(const tbc_batch* b);
/* PROGRESS of a run that is out (reference: knossos.search reports on a search while it runs -- knossos/src/knossos/search.clj, the
 * reporter its `run` starts; jepsen.checker/linearizable logs it).  Callable from ANOTHER thread while tbc_batch_run is in flight on
 * the batch (the one entry point that is; nothing else may touch a batch that is running): how many of the batch's histories have a
 * verdict so far -- the search kernels count them into host memory as they store their results --, the phase, the time since the
 * run began.  After the run: what it handed back (n_decided = the histories whose verdict is not TBC_UNKNOWN), running = 0. */
enum { TBC_PHASE_IDLE = 0, TBC_PHASE_PACK = 1 /* packing and the first search pass (queued together) */, TBC_PHASE_RETRIES = 2 /* verdicts
       composed; histories that overflowed, stalled or hit a budget are searched again */ };
typedef struct tbc_progress {
  uint32_t n_histories, n_decided, phase, running;
  uint64_t elapsed_ns;
} tbc_progress;
tbc_status tbc_batch_progress(const tbc_batch* b, tbc_progress* out);
/* how the last run was answered when the level sweep (knossos.linear; jit_sweep.hip) is in play:
 * TBC_ALG_LINEAR always asks for it, TBC_ALG_COMPETITION on small batches that want no witness.
 * The sweep cuts a history into segments of about seg_target completions at fronts with at most
 * cut_open open calls and sweeps them concurrently; histories it cannot finish (a config set
 * outgrows on-chip memory, > 64 process slots, set / bank) are answered by the depth-first
 * search instead -- tbc_result.analyzer says which (TBC_ALG_LINEAR = the sweep). */
typedef struct tbc_sweep_info {
  uint32_t enabled;       /* this batch runs the sweep first                              */
  uint32_t seg_target;    /* wanted segment length in completions (0 = one segment)       */
  uint32_t max_segs;      /* segments per history at most                                 */
  uint32_t cut_open;      /* a cut needs at most this many open calls                     */
  uint32_t n_dom;         /* states a segment may start in: nil + 0..greatest value of the batch */
  uint32_t n_segments;    /* last run: segments swept                                     */
  uint32_t n_fallback;    /* last run: histories handed to the depth-first search         */
} tbc_sweep_info;
tbc_status tbc_batch_sweep_info(const tbc_batch* b, tbc_sweep_info* out);

/* ---------------------------------------------- one history over several GPUs
 *
 * BASELINE.json's north_star asks for the search frontier of ONE history to be sharded over the
 * GPUs of a node.  With the level sweep that is a property of the algorithm: a history is a chain
 * of segments, every (segment, 32-origin slice) is swept by its own wavefront and hands on a
 * relation {origin -> origin ids of the next segment}; WHERE a wavefront runs does not matter.
 * So rank r of w sweeps the wavefronts with (segment * 4 + slice) % w == r
 * (tbc_batch_set_shard + tbc_batch_sweep_partial), the ranks exchange their relation tables --
 * ONE all-gather of tbc_batch_sweep_table() bytes over RCCL (jepsen-tigerbeetle_amd/shard.py),
 * entries a rank does not own are all zero, so the merged table is the bitwise OR -- and every rank
 * composes the merged table (tbc_batch_sweep_finish).  The inputs are replicated (a history is a
 * few hundred KB); pack runs on every rank.  A wavefront the sweep cannot finish (status 2) makes
 * the finishing rank fall back to its own depth-first search, as in the single-GPU path.
 */
#define TBC_SWEEP_SLICES 4u
typedef struct tbc_sweep_rel {   /* one per (history, segment, slice) */
  uint32_t status;               /* 0 = no such wavefront (or not this rank's), 1 = swept, 2 = overflow */
  uint32_t F0, F1;               /* levels swept: [F0, F1)                                         */
  uint32_t n_org;                /* origins of this slice that are configs                         */
  uint32_t max_level;            /* largest level                                                  */
  uint32_t subrounds;
  uint32_t n_end;                /* configs at front F1                                            */
  uint32_t end_state;            /* state of the first of them (non-register models)               */
  uint64_t configs_total;        /* sum of the level sizes                                         */
  uint64_t probes;               /* expansions                                                     */
  uint32_t M[32][TBC_SWEEP_SLICES]; /* M[o] = origin ids of the NEXT segment reachable from origin  */
                                 /* 32 * slice + o (128-bit set); last segment: word 0 = final states */
  uint32_t last_level[32];       /* greatest level at which a config reachable from origin o existed */
} tbc_sweep_rel;

typedef struct tbc_sweep_verdict {
  int32_t valid;                 /* TBC_VALID / TBC_INVALID / TBC_UNKNOWN (a wavefront missing or overflowed) */
  uint32_t fail_level;           /* invalid: rank of the completion nobody passes                  */
  uint32_t fail_seg;             /* invalid: the segment it lies in                                */
  uint32_t live_in[TBC_SWEEP_SLICES];  /* invalid: origin ids of that segment reachable from the start */
  uint32_t final_bits;           /* valid: final states reached (register family: nil = bit 0, v = bit v + 1) */
  uint32_t end_state;            /* valid, other models: the state                                 */
  uint32_t n_wavefronts;         /* relations composed                                             */
  uint64_t probes, configs_total, subrounds, max_level;
} tbc_sweep_verdict;

/* compose the relations of ONE history (max_segs * TBC_SWEEP_SLICES records, segment-major) in order.
 * Pure host code, no device needed. */
tbc_status tbc_sweep_compose(const tbc_sweep_rel* rel, uint32_t max_segs, uint32_t n_completions,
                             tbc_sweep_verdict* out);

tbc_status tbc_batch_set_shard(tbc_batch* b, uint32_t rank, uint32_t world);
/* pack + sweep of this rank's wavefronts; no verdicts yet */
tbc_status tbc_batch_sweep_partial(tbc_batch* b);
/* the relation table of the last partial run: DEVICE pointer (for a collective straight out of HBM) and size */
tbc_status tbc_batch_sweep_table(const tbc_batch* b, void** device_ptr, uint64_t* bytes);
/* verdicts from a merged relation table in HOST memory; merged_bytes must equal tbc_batch_sweep_table()'s size
 * (anything else is TBC_ERR_INVALID_ARG, as is a finish that no tbc_batch_sweep_partial precedes) */
tbc_status tbc_batch_sweep_finish(tbc_batch* b, const void* merged, uint64_t merged_bytes, tbc_result* results);
/* the same from the ranks' tables still in DEVICE memory, `world` of them back to back (what an all-gather over RCCL leaves):
 * they are OR-ed on the device into this batch's table, then composed -- the exchanged bytes never pass through the host */
tbc_status tbc_batch_sweep_merge(tbc_batch* b, const void* gathered_device, uint64_t gathered_bytes, uint32_t world, tbc_result* results);
/* ---- the exchange behind the C-ABI (round 6; csrc/tbc_comm.hip).  The host the reference is -- a Clojure process binding this library
 * through JNA (/root/reference/project.clj:6-8) -- has no torch.distributed; with these a rank of ANY host language runs its share
 * of a sharded check:
 *   tbc_comm_unique_id         rank 0: 128 bytes that reach the other ranks however the host likes (they are an ncclUniqueId)
 *   tbc_comm_init              an RCCL communicator over xGMI for this rank (librccl.so is loaded here, at the first call)
 *   tbc_comm_init_host         ... or a transport of the caller's: an all-gather over HOST memory (MPI, a socket, a test's gloo)
 *   tbc_batch_sweep_allgather  tbc_batch_set_shard + tbc_batch_sweep_partial + ONE all-gather of the relation tables (RCCL: straight
 *                              out of HBM, OR-merged on the device; host transport: through tbc_batch_sweep_finish) + composition.
 *                              Every rank calls it with a batch created from the same histories and options; every rank gets the results.
 */
typedef struct tbc_comm tbc_comm;
#define TBC_COMM_ID_BYTES 128
/* gather `bytes` from every rank: recv holds world * bytes, rank r's contribution at r * bytes.  0 = done. */
typedef int (*tbc_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes);
tbc_status tbc_comm_unique_id(void* id /* TBC_COMM_ID_BYTES */);
tbc_status tbc_comm_init(uint32_t rank, uint32_t world, const void* id, uint32_t device, tbc_comm** out);
tbc_status tbc_comm_init_host(uint32_t rank, uint32_t world, tbc_allgather_fn fn, void* user, tbc_comm** out);
uint32_t tbc_comm_rank(const tbc_comm* c);
uint32_t tbc_comm_world(const tbc_comm* c);
void tbc_comm_destroy(tbc_comm* c);
tbc_status tbc_batch_sweep_allgather(tbc_batch* b, tbc_comm* c, tbc_result* results);
void tbc_batch_destroy(tbc_batch* b);

/* ------------------------------------------------ streaming: the same batch, fresh histories
 *
 * The reference calls a checker ONCE per history: checker/compose over the test's one history
 * (/root/reference/src/tigerbeetle/core.clj:139-146), jepsen.independent/checker once per key
 * (/root/reference/src/tigerbeetle/workloads/set_full.clj:155-158).  A caller that checks many histories
 * never checks one twice, and creating a batch per input pays for 85 GB of allocation, the op columns
 * over PCIe from pageable memory and a sizing pass every time (round 5: 12-22k histories/s against 321k
 * resident).  These entry points keep a batch -- arenas, streams, the decisions tbc_batch_create made --
 * and change its histories:
 *
 *   tbc_batch_map_input     a slot of library-owned PINNED host memory for the caller to fill IN PLACE (a JNA
 *                           Memory / direct ByteBuffer / numpy view over it): no copy inside the library
 *   tbc_batch_submit_input  queues the slot's copy to the device on the batch's copy stream and returns; it runs
 *                           under whatever the batch (or another batch) is computing.  Up to two inputs may wait.
 *   tbc_batch_run           consumes the oldest waiting input, if any (else the resident input once more): waits
 *                           for its copy, unpacks it on the device, packs, searches.  results: n_hist of THAT input.
 *   tbc_batch_reload        convenience: the six columns of a tbc_batch_desc -> wire format -> slot 0 / 1 -> submitted
 *
 * WIRE FORMAT, 12 B an op (21 B in tbc_ops): word = f | a << 4 | b << 12 | process << 20 (f 4 bits; a, b 8 bits:
 * 0..254 or TBC_WIRE_NIL; process 12 bits), inv_pos, ret_pos as in tbc_ops.  Register / cas-register / mutex.
 *
 * What a fresh input must share with the input the batch was created from (else TBC_ERR_UNSUPPORTED from the call
 * that finds out -- tbc_batch_submit_input or the tbc_batch_run that consumes it -- and the caller destroys and
 * creates): at most the first input's number of histories and an eighth more than its ops; process slots within the
 * batch's mask words; register values within the batch's value domain (the greatest value of the first input,
 * when the dominance rules are on); no crashed call if the first input had none.  A COUNT-FORM batch (created from
 * histories with crashed calls that have an effect, under the default rules: what a nemesis makes) takes fresh inputs
 * too: the classes of crashed calls and the re-used process slots are planned on the host inside
 * tbc_batch_submit_input (a few host threads; the caller's words are not modified), and an input whose crashed calls
 * do not fit the form (> 128 bits of counts) is refused.  Batches of the level sweep (incl. a count-form batch of
 * <= 8 histories, which has the relaxed sweep beside it), of set / bank / multi-register / table models and the
 * sequential schedule take no fresh inputs.
 * Verdict, failing op and every counter of a consumed input equal those of a batch created from the same histories
 * (tests/test_stream_gpu.py).
 */
#define TBC_WIRE_NIL 0xFFu
#define TBC_WIRE_WORD(f, a8, b8, process) ((uint32_t)(f) | ((uint32_t)(a8) << 4) | ((uint32_t)(b8) << 12) | ((uint32_t)(process) << 20))

typedef struct tbc_batch_input {   /* pointers into one pinned slot; valid until the batch is destroyed */
  uint32_t n_hist_cap;            /* histories the slot holds at most                              */
  uint32_t reserved0;
  uint64_t ops_cap;               /* ops the slot holds at most                                    */
  uint64_t* op_off;               /* [n_hist_cap + 1] as tbc_batch_desc.op_off                     */
  uint32_t* n_events;             /* [n_hist_cap]                                                  */
  uint32_t* n_process;            /* [n_hist_cap]                                                  */
  uint32_t* word;                 /* [ops_cap] TBC_WIRE_WORD(f, a, b, process)                     */
  uint32_t* inv_pos;              /* [ops_cap]                                                     */
  uint32_t* ret_pos;              /* [ops_cap] TBC_POS_CRASHED = never completed                   */
} tbc_batch_input;

/* slot < 16; allocated when first mapped.  Waits until the slot's previous input has left for the device. */
tbc_status tbc_batch_map_input(tbc_batch* b, uint32_t slot, tbc_batch_input* out);
/* the slot holds n_hist histories (op_off[0..n_hist], n_events, n_process, the wire columns): copy them, asynchronously */
tbc_status tbc_batch_submit_input(tbc_batch* b, uint32_t slot, uint32_t n_hist);
tbc_status tbc_batch_reload(tbc_batch* b, const tbc_batch_desc* desc);

typedef struct tbc_input_info {
  uint32_t n_hist;                /* histories of the resident input (what tbc_batch_run's results hold) */
  uint32_t pending;               /* submitted inputs not yet consumed                                  */
  uint64_t total_ops;             /* ops of the resident input                                          */
  uint64_t bytes_copied;          /* last consumed input: bytes that crossed PCIe ...                   */
  uint64_t ns_copy;               /* ... and how long the copy took (HIP events on the copy stream)     */
  uint64_t inputs_consumed;
  uint32_t lists_regrown;         /* times an input's per-front lists outgrew their arena               */
  uint32_t n_hist_cap;
  uint64_t ops_cap;
} tbc_input_info;
tbc_status tbc_batch_input_info(const tbc_batch* b, tbc_input_info* out);

/* ----------------------------------------------------------------- memo
 *
 * knossos.model.memo/memo for a caller-defined model: given the closure
 * step(state, class) over n_classes op classes, enumerate reachable states
 * breadth-first from state 0 and fill a dense table.  `step` returns the next
 * state id handle or -1 for inconsistent; ids are opaque int64 handles chosen
 * by the caller (for example a packed value).  Host only.
 */
typedef int64_t (*tbc_step_fn)(int64_t state, uint32_t op_class, void* user);
tbc_status tbc_memo_build(int64_t init_state, uint32_t n_classes,
                          tbc_step_fn step, void* user, uint32_t max_states,
                          uint16_t* table /* max_states*n_classes */,
                          int64_t* state_handles /* max_states */,
                          uint32_t* n_states);

/* ------------------------------------------------------- checker/set-full
 *
 * jepsen.checker/set-full -- the checker the reference actually runs for its set-full workload
 * (/root/reference/src/tigerbeetle/workloads/set_full.clj:157, `(checker/set-full {:linearizable? true})`;
 * SURVEY.md section 8f row 3).  Per element of the set three history indices decide everything
 * (recalled from jepsen.checker; restated in oracle/set_full.py):
 *   known         first op that proved the element exists: its add's :ok, or the :ok of a read containing it
 *   last_present  invocation of the latest-invoked :ok read that contained it
 *   last_absent   invocation of the latest-invoked :ok read that did not
 * (only reads completing after the element's add was invoked count).  The device part is the scan of the
 * reads x elements membership matrix that yields those three per element -- a streaming pass, the one
 * kernel on this path with a real HBM roofline.  tbc_setfull_run hands those three indices back; tbc_setfull_results
 * (below) goes on to decide outcomes (:stable / :lost / :never-read), latencies, counts, :valid?, latency quantiles
 * and the worst stale elements on the device and returns the check result.
 *
 * Inputs (caller-owned): elements numbered in order of their first :add invocation (add_invoke ascending),
 * reads = the :ok reads in order of invocation (read_invoke ascending); present = n_reads rows of
 * words_per_row 32-bit words, bit e of row r = read r's value contains element e.
 */
typedef struct tbc_setfull_in {
  uint32_t n_elements, n_reads, words_per_row, device;
  const uint32_t* add_invoke;    /* [n_elements] history index of the element's :add invocation  */
  const uint32_t* add_ok;        /* [n_elements] index of that add's :ok, TBC_NO_OP if none      */
  const uint32_t* read_invoke;   /* [n_reads]                                                    */
  const uint32_t* read_ok;       /* [n_reads]                                                    */
  const uint32_t* present;       /* [n_reads * words_per_row]                                    */
} tbc_setfull_in;

typedef struct tbc_setfull_out {   /* arrays caller-allocated, n_elements each; TBC_NO_OP = none */
  uint32_t* known;
  uint32_t* last_present;
  uint32_t* last_absent;
  uint64_t ns_scan;              /* device time of the scan kernel (HIP events)                  */
  uint64_t bytes_scanned;        /* matrix bytes the scan loaded                                 */
  uint64_t bytes_matrix;         /* n_reads * words_per_row * 4                                  */
} tbc_setfull_out;

typedef struct tbc_setfull tbc_setfull;
/* inputs become resident in HBM (H2D here); run scans them; results copied into `out`.  All three creates (this one, _create_rows,
 * tbc_setfull_keys_create) check every rule of their input on the host before any device call: TBC_ERR_INVALID_ARG, the message names
 * the entry point.  words_per_row may exceed ceil(n_elements / 32): the extra words of a row are ignored. */
tbc_status tbc_setfull_create(const tbc_setfull_in* in, tbc_setfull** handle);

/* The same with the reads in COMPACT form, the membership matrix built ON THE DEVICE (nothing of size reads x elements exists on
 * the host or crosses PCIe).  A read of a grow-only set is, up to a few exceptions, a PREFIX of the elements in add-invocation
 * order -- what had been added when it ran; so read r is given as top[r] (every element numbered below top[r] is in it) and a
 * list of exceptions exc[exc_off[r] .. exc_off[r + 1]): element numbers, each at most once per read -- a listed element below
 * top[r] is ABSENT from the read, one at or above it PRESENT.  (The reference's reads, workloads/set_full.clj:128-134, return the
 * sorted set: the caller numbers the values by add invocation, takes top = greatest element read + 1 and lists the holes.) */
typedef struct tbc_setfull_rows {
  uint32_t n_elements, n_reads, device, reserved0;
  const uint32_t* add_invoke;    /* as tbc_setfull_in */
  const uint32_t* add_ok;
  const uint32_t* read_invoke;
  const uint32_t* read_ok;
  const uint32_t* top;           /* [n_reads], <= n_elements */
  const uint64_t* exc_off;       /* [n_reads + 1], ascending, exc_off[0] = 0 */
  const uint32_t* exc;           /* [exc_off[n_reads]] element numbers < n_elements, each at most once per read, in any order (a duplicate is TBC_ERR_INVALID_ARG) */
} tbc_setfull_rows;
tbc_status tbc_setfull_create_rows(const tbc_setfull_rows* in, tbc_setfull** handle);
tbc_status tbc_setfull_run(tbc_setfull* handle, tbc_setfull_out* out);
void tbc_setfull_destroy(tbc_setfull* handle);

/* Many keys of one independent history (jepsen.independent, set_full.clj:155) in ONE object: every key in the compact form of
 * tbc_setfull_rows, the arrays of all keys laid end to end, key after key.  Element and read numbers stay LOCAL to their key (top,
 * exc and each key's orders exactly as tbc_setfull_rows); exc_off runs over the whole input (exc_off[0] = 0, ascending).  Each call
 * does a fixed number of launches and copies whatever n_keys is.  Every rule is checked on the host before any device work; an error
 * names the key (and the read).  Keys with no element or no read are allowed (no read: known = the add's :ok, nothing seen). */
typedef struct tbc_setfull_keys_in {
  uint32_t n_keys, device;
  const uint32_t* n_elements;    /* [n_keys] */
  const uint32_t* n_reads;       /* [n_keys] */
  const uint32_t* add_invoke;    /* [sum n_elements], key after key; per key as tbc_setfull_rows */
  const uint32_t* add_ok;
  const uint32_t* read_invoke;   /* [sum n_reads], key after key */
  const uint32_t* read_ok;
  const uint32_t* top;           /* [sum n_reads], element numbers local to the row's key */
  const uint64_t* exc_off;       /* [sum n_reads + 1], offsets into exc over the whole input */
  const uint32_t* exc;           /* element numbers local to the row's key */
} tbc_setfull_keys_in;
typedef struct tbc_setfull_keys_out {          /* [sum n_elements] each, key after key; TBC_NO_OP = none */
  uint32_t *known, *last_present, *last_absent;
  uint64_t ns_scan, bytes_scanned, bytes_matrix;
} tbc_setfull_keys_out;
typedef struct tbc_setfull_keys tbc_setfull_keys;
tbc_status tbc_setfull_keys_create(const tbc_setfull_keys_in* in, tbc_setfull_keys** handle);
tbc_status tbc_setfull_keys_run(tbc_setfull_keys* handle, tbc_setfull_keys_out* out);
void tbc_setfull_keys_destroy(tbc_setfull_keys* handle);

/* The check result itself, decided on the device: tbc_setfull_results / tbc_setfull_keys_results scan (exactly what _run does) and then
 * turn the three indices -- which stay on the device -- into every element's outcome and latencies and every key's counts, :valid?,
 * latency quantiles and worst stale elements (csrc/set_full_results.h).  A fixed number of launches whatever n_keys is.  Semantics as
 * oracle/set_full.py `outcomes` and `check`, all in 64-bit integers:
 *   stable  <=> last_present exists and last_absent < last_present
 *   lost    <=> known, last_absent exists, last_present < last_absent and known < last_absent;  otherwise never-read
 *   stable_latency = max(0, (time[last_absent] + 1, or 0 if there is none) - time[known]) / unit;  lost_latency likewise from last_present
 *   stale   <=> stable and stable_latency > 0
 *   valid: false if anything is lost, else unknown if nothing is stable, else false if TBC_SETFULL_F_LINEARIZABLE and something is stale,
 *          else true.  Duplicated elements are found by the caller's encoder and are NOT known here: the caller ANDs them in
 *          (any duplicate makes the result false).
 *   quantile p of n values = the value at rank min(n - 1, (uint64_t)((double)n * p)) of the ascending order
 *   worst stale = the 8 greatest stable latencies among stale elements, equal latencies by ascending element number.
 * Times: op_time[time_off[k] + i] is the :time of key k's op i -- i the same local op index add_invoke, add_ok, read_invoke and read_ok
 * use; slots of other ops may hold anything; time differences must fit an int64.  Each key's slice must be longer than the greatest
 * index among the key's inputs.  op_time == NULL: time = the op index and unit 1 (time_off is not read).  A short slice, a null
 * argument or unit == 0 is TBC_ERR_INVALID_ARG before any device work; the message names the entry point and the key. */
#define TBC_SETFULL_F_LINEARIZABLE 1u
enum { TBC_SETFULL_NEVER_READ = 0, TBC_SETFULL_STABLE = 1, TBC_SETFULL_LOST = 2 };            /* outcome */
enum { TBC_SETFULL_VALID_FALSE = 0, TBC_SETFULL_VALID_TRUE = 1, TBC_SETFULL_VALID_UNKNOWN = 2 };
#define TBC_SETFULL_WORST 8
typedef struct tbc_setfull_times {
  const int64_t* op_time;        /* [time_off[n_keys]] or NULL */
  const uint64_t* time_off;      /* [n_keys + 1], ascending (one key: {0, n_ops}) */
  uint64_t unit;                 /* 1,000,000 for jepsen's ns -> whole ms, or 1; never 0 */
  uint32_t flags, reserved0;     /* TBC_SETFULL_F_* */
} tbc_setfull_times;
typedef struct tbc_setfull_key_summary {
  uint32_t attempt_count, stable_count, lost_count, never_read_count, stale_count;
  uint8_t valid;                                     /* TBC_SETFULL_VALID_* (duplicates not counted in: see above) */
  uint8_t stable_q_present, lost_q_present;          /* 1: the five points below hold values (the count is not 0) */
  uint8_t n_worst;                                   /* <= TBC_SETFULL_WORST */
  int64_t stable_q[5], lost_q[5];                    /* the points {0, .5, .95, .99, 1} */
  uint32_t worst_element[TBC_SETFULL_WORST];         /* element numbers local to the key, worst first */
  uint32_t worst_known[TBC_SETFULL_WORST];           /* their known and last_absent (TBC_NO_OP = none) */
  uint32_t worst_last_absent[TBC_SETFULL_WORST];
  int64_t worst_latency[TBC_SETFULL_WORST];
} tbc_setfull_key_summary;
typedef struct tbc_setfull_results_out {             /* arrays caller-allocated, [sum n_elements] each, key after key */
  uint8_t* outcome;                                  /* TBC_SETFULL_NEVER_READ / _STABLE / _LOST */
  int64_t* stable_latency;                           /* -1 where the element is not stable */
  int64_t* lost_latency;                             /* -1 where it is not lost */
  uint32_t *known, *last_present, *last_absent;      /* each optional: NULL = not wanted */
  tbc_setfull_key_summary* summary;                  /* [n_keys] */
  uint64_t ns_scan;                                  /* as tbc_setfull_out */
  uint64_t ns_results;                               /* device time of the kernels after the scan (HIP events) */
  uint64_t bytes_scanned, bytes_matrix;
} tbc_setfull_results_out;
tbc_status tbc_setfull_results(tbc_setfull* handle, const tbc_setfull_times* times, tbc_setfull_results_out* out);
tbc_status tbc_setfull_keys_results(tbc_setfull_keys* handle, const tbc_setfull_times* times, tbc_setfull_results_out* out);

/* The history itself, as op columns: tbc_setfull_keys_create_ops takes each key's client ops (in history order) and the raw values of
 * its reads, and encodes them here -- the caller flattens nothing and knows none of set-full's rules.  The host plans the O(ops) part
 * (csrc/set_full_encode_plan.h): which value is which column, which :ok read belongs to which invocation.  The device does the
 * O(values) part (csrc/set_full_encode.h): every value of every read is looked up in a hash table of its key's elements and its bit
 * set in the read's row; duplicates are found on the way.  The handle is an ordinary tbc_setfull_keys: _run, _results and _destroy work
 * on it unchanged, and its matrix is bit for bit the one tbc_setfull_keys_create builds from the compact form of the same history.
 * A single history is n_keys = 1.
 *   elements  an element is a distinct :add value.  An :add INVOCATION starts the element afresh: an element added again is numbered
 *             by its LAST add invocation; elements are numbered in the order of those.  add_ok = the first :ok add of the value after
 *             that invocation, from any process; an :ok add of a value never invoked is ignored.  An :add with TBC_SETFULL_T_NIL is
 *             skipped.
 *   reads     an :ok read is paired with the open read invocation of its process; a :fail closes it; an :info leaves it open until
 *             the process invokes a read again.  An :ok read with TBC_SETFULL_T_NIL, or without an open invocation, closes the open
 *             read and is no read; one with an empty value is a read that saw nothing.  Reads are numbered by invocation.  A value
 *             that names no element of the key is not a column: it is counted in unknown_values and otherwise ignored.
 * Every rule of the struct is checked on the host before any device call -- non-null pointers, op_off ascending, index strictly
 * ascending within a key (and never TBC_NO_OP), val_off ascending from 0, type and f in range: TBC_ERR_INVALID_ARG, the message names
 * the entry point, the key and the op.  Valid input without a gfx950 device: TBC_ERR_NO_DEVICE (no CPU fallback). */
enum { TBC_SETFULL_T_INVOKE = 0, TBC_SETFULL_T_OK = 1, TBC_SETFULL_T_FAIL = 2, TBC_SETFULL_T_INFO = 3 };
#define TBC_SETFULL_T_NIL 0x80u          /* or-ed into type: the op's :value is nil */
enum { TBC_SETFULL_OP_OTHER = 0, TBC_SETFULL_OP_ADD = 1, TBC_SETFULL_OP_READ = 2 };
/* A read's row is assembled in a window of this many 32-bit words of LDS (csrc/set_full_encode.h); a key of more than 32 x this many
 * elements takes one pass over the read's values per window. */
#define TBC_SETFULL_ENCODE_WINDOW_WORDS 8192u

typedef struct tbc_setfull_ops_in {
  uint32_t n_keys, device;
  const uint64_t* op_off;   /* [n_keys + 1] key k's client ops are rows op_off[k] .. op_off[k+1], in history order */
  const uint32_t* index;    /* [n_ops] the op's index in ITS KEY's history (what add_invoke ... are numbered by); strictly ascending per key */
  const uint8_t*  type;     /* TBC_SETFULL_T_* (| TBC_SETFULL_T_NIL) */
  const uint8_t*  f;        /* TBC_SETFULL_OP_* ; OTHER is skipped */
  const int64_t*  process;
  const int64_t*  value;    /* an :add's element; not read for other ops */
  const uint64_t* val_off;  /* [n_ops + 1] ascending, val_off[0] = 0: vals[val_off[i] .. val_off[i+1]) = the value of op i if it is an :ok read, else empty */
  const int64_t*  vals;     /* the reads' values, in any order, repeats allowed */
} tbc_setfull_ops_in;
tbc_status tbc_setfull_keys_create_ops(const tbc_setfull_ops_in* in, tbc_setfull_keys** handle);

/* The sums over the object's keys of n_elements and n_reads: what the arrays of tbc_setfull_keys_out, tbc_setfull_results_out and
 * tbc_setfull_encoding are sized by.  Works on every keyed handle, however it was made. */
tbc_status tbc_setfull_keys_shape(tbc_setfull_keys* h, uint64_t* sum_elements, uint64_t* sum_reads);

/* What tbc_setfull_keys_create_ops made of the ops: the encoding (what a caller of tbc_setfull_keys_create would have had to compute)
 * and the two things only the raw values show.
 *   dup_max / dup_count   an element that occurs more than once in ONE read's value is a duplicate.  dup_count[k] != 0 MAKES KEY k's
 *                         RESULT FALSE, whatever tbc_setfull_key_summary.valid says: the summary's verdict keeps its documented
 *                         meaning (duplicates not counted in), and the caller ANDs `dup_count[k] == 0` into it.
 *   unknown_values        read values that name no element of the key.  They are not columns and do not enter the scan.  DUPLICATES
 *                         AMONG THEM ARE NOT SEEN by the library (dup_max has a slot per element only): a caller that wants jepsen's
 *                         `duplicated` in full counts the repeats among a key's unknown values itself -- only keys with
 *                         unknown_values[k] != 0 can have any.
 * On a handle that was not made by tbc_setfull_keys_create_ops: TBC_ERR_INVALID_ARG (the message says that the object was not made
 * from ops). */
typedef struct tbc_setfull_encoding {          /* every pointer optional (NULL = not wanted); caller-allocated */
  uint32_t *n_elements, *n_reads;              /* [n_keys] */
  int64_t*  element;                           /* [sum_elements] the value of each column, key after key */
  uint32_t *add_invoke, *add_ok;               /* [sum_elements] */
  uint32_t *read_invoke, *read_ok;             /* [sum_reads] */
  uint32_t* dup_max;                           /* [sum_elements] greatest multiplicity of the element within ONE read (0 or 1: not duplicated) */
  uint32_t* dup_count;                         /* [n_keys] elements with dup_max > 1 */
  uint64_t* unknown_values;                    /* [n_keys] read values that name no element of the key */
  uint64_t  ns_encode;                         /* device time of the encoding kernels at create (HIP events) */
} tbc_setfull_encoding;
tbc_status tbc_setfull_keys_encoding(tbc_setfull_keys* h, tbc_setfull_encoding* out);

/* ----------------------------------------------------------------- ledger */
/* The ledger workload's checkers (the reference's tests/ledger.clj:154-282, composed at :363-367) from the history as op columns, in ONE
 * call: the bank checker (:SI), lookup-all-invoked-transfers and final-reads.  (unexpected-ops returns ops and is O(ops): the caller's.)
 * The caller flattens the client ops (integer :process, history order) and their micro-ops [f id {..}]; the host plans the O(ops) part
 * (csrc/ledger_plan.h: which op is which row, the distinct invoked transfer ids), the device does everything that is O(micro-ops)
 * (csrc/ledger_kernels.h).  All arithmetic is in 64-bit integers; the caller keeps a read's sum of |credits| + |debits| plus
 * |total_amount| below 2^63 (jepsen/ledger.py LedgerColumns refuses more), so no sum wraps.
 *
 * Rows.  Reads are numbered in history order among the ops with type == OK && kind == READ; final reads and final lookups likewise
 * among the ops that are OK, of their kind, and FINAL.  The caller sizes the output arrays from its own columns.
 *
 * SI, per OK read: the balance of a micro-op is a - b (credits-posted - debits-posted), nil under TBC_LEDGER_M_NIL;
 *   unexpected = its micro-ops whose id is no account, nil = those whose balance is nil, total = the sum of the non-nil balances of ALL
 *   its micro-ops.  read_error is the first that holds, in check-op's cond order: 1 unexpected-key (unexpected > 0), 2 nil-balance,
 *   3 wrong-total (total != total_amount), 4 negative-value (!negative_balances and some balance < 0), else 0.  read_badness by type:
 *   1 unexpected, 2 nil, 3 |total - total_amount|, 4 -(the sum of the negative balances).
 *   THIS DEPARTS FROM THE REFERENCE ON PURPOSE: its err-badness of a wrong total is (float (/ (- total expected) expected)), which throws
 *   with the reference's own default :total-amount 0 and collapses near values to equal floats; the integer distance picks the same
 *   worst op wherever that float is defined and distinct.
 *   Per type: count, first and last (read numbers), worst = the read of the greatest badness; for wrong-total also lowest / highest =
 *   the reads of the least / greatest total.  Ties go to the EARLIEST read (jepsen.util/max-by, min-by: only a strictly greater element
 *   replaces the held one).  first_error = the least read number with an error; valid_si = no error.
 * lookup-transfers: T = the distinct ids of all micro-ops of the ops with INVOKE && kind == TRANSFER.  lookup_missing[l] = |T| - |T and
 *   the ids of final lookup l| (repeated ids count once, ids nobody invoked not at all); suspect_lookups = the rows with missing > 0;
 *   valid_lookups = none.
 * final-reads: a final row is UNLIKE when its micro-ops are not the first final row's: the same count and, position by position, the
 *   same id, a, b, c, flags (vector equality: order matters).  valid_final_reads = n_final_reads >= 1 && n_final_lookups >= 1 && nothing
 *   unlike (no final row at all is the reference's (not= 1 (count ...))).
 *
 * Every rule of the struct is checked on the host before any device call -- non-null pointers, mop_off ascending from 0, index strictly
 * ascending (and never TBC_NO_OP), type, kind and the op flags in range, accounts distinct, and within each OK read the micro-op flags
 * in range and the ids distinct: TBC_ERR_INVALID_ARG, the message names the entry point and the op.  The micro-ops of transfers and
 * lookups are never looked at on the host: their flag bytes are compared as they are (final-reads) and otherwise not read.  Valid input without a gfx950 device: TBC_ERR_NO_DEVICE (no CPU
 * fallback).  One-shot and re-entrant: one device allocation, a stream and events of its own, all gone on every path out, and the
 * calling thread's current device as it was; columns that do not fit the device: TBC_ERR_OOM. */
enum { TBC_LEDGER_T_INVOKE = 0, TBC_LEDGER_T_OK = 1, TBC_LEDGER_T_FAIL = 2, TBC_LEDGER_T_INFO = 3 };
enum { TBC_LEDGER_K_OTHER = 0, TBC_LEDGER_K_TRANSFER = 1, TBC_LEDGER_K_READ = 2, TBC_LEDGER_K_LOOKUP = 3 }; /* f of the op's FIRST micro-op (op->txn-f) */
#define TBC_LEDGER_F_FINAL 1u   /* op flag: :final? */
#define TBC_LEDGER_M_NIL   1u   /* micro-op flag: its third element is nil */
enum { TBC_LEDGER_E_NONE = 0, TBC_LEDGER_E_UNEXPECTED_KEY = 1, TBC_LEDGER_E_NIL_BALANCE = 2, TBC_LEDGER_E_WRONG_TOTAL = 3, TBC_LEDGER_E_NEGATIVE_VALUE = 4 };
/* A final lookup's transfer numbers are gathered in a window of this many 32-bit words of LDS (csrc/ledger_kernels.h); more than 32 x
 * this many invoked transfers take one pass over the lookup's ids per window. */
#define TBC_LEDGER_LOOKUP_WINDOW_WORDS 8192u

typedef struct tbc_ledger_in {
  uint32_t n_ops, device;                 /* client ops (integer :process) in history order */
  const uint32_t* index;                  /* strictly ascending, never TBC_NO_OP */
  const uint8_t *type, *kind, *flags;
  const uint64_t* mop_off;                /* [n_ops + 1] ascending from 0 */
  const int64_t *mop_id, *mop_a, *mop_b, *mop_c;  /* :r  a = credits-posted, b = debits-posted;  :t / :l-t  a = debit-acct, b = credit-acct, c = amount */
  const uint8_t* mop_flags;
  const int64_t* accounts; uint32_t n_accounts; uint32_t negative_balances;   /* accounts in any order, distinct */
  int64_t total_amount;
} tbc_ledger_in;

typedef struct tbc_ledger_errors {        /* one error type: read numbers, TBC_NO_OP where there is none */
  uint32_t count, first, last, worst;
} tbc_ledger_errors;

typedef struct tbc_ledger_summary {
  uint32_t read_count, error_count, first_error;      /* first_error: a read number, TBC_NO_OP if none */
  uint32_t lowest, highest;                           /* wrong-total: the reads of the least / greatest total */
  uint32_t n_transfers;                               /* |T| */
  tbc_ledger_errors errors[5];                        /* [TBC_LEDGER_E_*]; [0] is not used */
  uint32_t n_final_reads, final_reads_unlike;
  uint32_t n_final_lookups, final_lookups_unlike, suspect_lookups;
  uint8_t valid_si, valid_lookups, valid_final_reads, reserved0;
  uint64_t ns_device;                                 /* the kernels, between HIP events */
  uint64_t bytes_in;                                  /* copied to the device */
} tbc_ledger_summary;

typedef struct tbc_ledger_out {           /* arrays caller-allocated, each optional (NULL = not wanted) */
  uint8_t* read_error;                    /* [n_ok_reads] TBC_LEDGER_E_* */
  int64_t *read_total, *read_badness;     /* [n_ok_reads] (badness: 0 where there is no error) */
  uint32_t* lookup_missing;               /* [n_final_lookups] */
  uint8_t *final_read_unlike, *final_lookup_unlike;   /* [n_final_reads], [n_final_lookups]: 1 = not the first row's micro-ops */
  tbc_ledger_summary summary;
} tbc_ledger_out;
tbc_status tbc_ledger_check(const tbc_ledger_in* in, tbc_ledger_out* out);

/* ------------------------------------------------------------------- ledger: realtime bounds on the posted counters
 * credits-posted and debits-posted of an account only grow, so every counter an :ok read returns has three bounds in real time: at least
 * what the transfers that had completed :ok before the read was invoked add up to (else the read is STALE), at most what the transfers
 * invoked before the read completed add up to (FUTURE), at least what any read that completed before its invocation saw (REGRESSED) --
 * a necessary condition for strict serializability in O(n log n).  THE RULES ARE STATED ONCE, in the docstring of jepsen/ledger.py
 * ("Realtime bounds"): transfers, reads, checked micro-ops, lo / hi / floor, the bits, the misses, the summary, the ranges.
 * Input: a tbc_ledger_in (total_amount and negative_balances are not used) plus
 *   process             [n_ops] the op's :process: pairing is knossos.history/pair-index, by process, as tbc_perf_series pairs
 *   init_credits/debits [n_accounts] the counters' initial values in the order of `accounts`, |x| < 2^61; NULL = zeros
 *   ok_transfers_apply  0 or 1: whether an :ok transfer is known to have been applied (the lower bound counts it)
 * Rows: reads are numbered as for tbc_ledger_check; read micro-ops in the order of the columns, over the OK reads.
 *   rt_bits[r]       1 stale credits, 2 stale debits, 4 future credits, 8 future debits, 16 regressed credits, 32 regressed debits
 *   rt_miss[r][k]    k = TBC_LEDGER_RT_STALE / FUTURE / REGRESSED: the greatest miss of that kind over the read's micro-ops and both
 *                    fields, saturating at INT64_MAX; 0 if there is none
 *   mop_lo/hi/floor[m][x]  x = 0 credits-posted, 1 debits-posted: the bounds of read micro-op m, all INT64_MIN where it is not checked
 *                    (nil, or its id no account); floor is INT64_MIN where no earlier read checked the account
 * The host plans what is O(ops) (csrc/ledger_rt_plan.h) and never reads a transfer's micro-ops; the device does the rest
 * (csrc/ledger_rt_kernels.h).  Every rule of tbc_ledger_in, and process non-null, |init| < 2^61, ok_transfers_apply in range, fewer
 * than 2^31 micro-ops of transfers and of reads: TBC_ERR_INVALID_ARG before any device call, the message names the entry point and the
 * op.  An amount outside [0, 2^31) among the micro-ops of the transfers that did not fail is counted ON THE DEVICE:
 * TBC_ERR_UNSUPPORTED, no results, summary.bad_amounts says how many.  No gfx950 device: TBC_ERR_NO_DEVICE.  One-shot and
 * re-entrant as tbc_ledger_check is. */
enum { TBC_LEDGER_RT_STALE = 0, TBC_LEDGER_RT_FUTURE = 1, TBC_LEDGER_RT_REGRESSED = 2 };

typedef struct tbc_ledger_rt_in {
  tbc_ledger_in ledger;
  const int32_t* process;                 /* [n_ops] */
  const int64_t *init_credits, *init_debits;  /* [n_accounts], NULL = zeros */
  uint32_t ok_transfers_apply, reserved0;
} tbc_ledger_rt_in;

typedef struct tbc_ledger_rt_summary {
  uint32_t read_count, error_count, first_error, valid;   /* error_count: reads with any bit; first_error: TBC_NO_OP if none */
  tbc_ledger_errors errors[3];                            /* [TBC_LEDGER_RT_*]: read numbers; worst = the greatest miss, ties the earliest */
  uint32_t n_definite, n_possible;                        /* transfers that completed :ok; transfers that did not fail */
  uint32_t foreign_sides;                                 /* sides of the micro-ops of the transfers that did not fail that name no account (a nil micro-op: both); skipped */
  uint32_t bad_amounts;                                   /* amounts outside [0, 2^31) among them */
  uint64_t n_checked;                                     /* read micro-ops checked */
  uint64_t ns_device;                                     /* the kernels, between HIP events */
  uint64_t bytes_in;                                      /* copied to the device */
} tbc_ledger_rt_summary;

typedef struct tbc_ledger_rt_out {        /* arrays caller-allocated, each optional (NULL = not wanted) */
  uint8_t* rt_bits;                       /* [n_ok_reads] */
  int64_t* rt_miss;                       /* [n_ok_reads][3] */
  int64_t *mop_lo, *mop_hi, *mop_floor;   /* [n_read_mops][2] */
  tbc_ledger_rt_summary summary;
} tbc_ledger_rt_out;
tbc_status tbc_ledger_realtime(const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out);

/* ------------------------------------------------------------------- ledger: reads as snapshots in one order
 * credits-posted and debits-posted only grow and the workload's reads read every account, so under serializability the reads of a
 * history are a CHAIN under component-wise <=.  Two reads are SKEWED when each is below the other on some counter (a long fork: the
 * 2-cycle of the monotonic-key graph); with every read complete, "no read skewed" plus "no read regressed" (tbc_ledger_realtime) holds
 * exactly when the graph of monotonic-key and realtime edges over the reads is acyclic.  THE RULES ARE STATED ONCE, in the docstring of
 * jepsen/ledger.py ("Snapshot order"): reads, checked micro-ops, counters, complete / partial, below, skewed, the summary, the ranges.
 * Input: a plain tbc_ledger_in (total_amount and negative_balances are not used; no process column: real time is
 * tbc_ledger_realtime's business).  Rows: reads are numbered as for tbc_ledger_check.  A counter is 2 x (the account's position in
 * `accounts`) + (0 credits-posted, 1 debits-posted).
 *   skew_count[r]    the reads r is skewed with
 *   skew_first[r]    the least read number among them, TBC_NO_OP if none
 *   skew_key[r][2]   against that first partner: the least counter on which r is below it, the least on which r is above it; TBC_NO_OP
 *   snap_flags[r]    TBC_LEDGER_SNAP_PARTIAL (the read does not check every account) | TBC_LEDGER_SNAP_SKEWED
 * The host plans what is O(ops) (csrc/ledger_snap_plan.h) and reads no micro-op beyond the validation of the reads' own; only the reads'
 * id, a, b and flags are copied (25 bytes a micro-op).  The device lays the reads out densely, sorts them by (sum, read number), scans
 * prefix maxima and suffix minima per counter to find the CANDIDATES -- the partial reads, and the complete reads skewed with a complete
 * read -- and compares only those with every read (csrc/ledger_snap_kernels.h): a history without candidates launches no pair kernel.
 * Every rule of tbc_ledger_in: TBC_ERR_INVALID_ARG before any device call, and so are reads x counters >= 2^31 and 2^31 micro-ops of
 * reads in one call.  The whole int64 range of a counter works, negative values included; a read whose sum of |v| over its checked
 * counters reaches 2^63 is counted ON THE DEVICE: TBC_ERR_UNSUPPORTED, no results, summary.bad_values says how many.  No gfx950 device:
 * TBC_ERR_NO_DEVICE.  One-shot and re-entrant as tbc_ledger_check is. */
#define TBC_LEDGER_SNAP_PARTIAL 1u
#define TBC_LEDGER_SNAP_SKEWED  2u

typedef struct tbc_ledger_snap_summary {
  uint32_t read_count, n_partial, valid, bad_values;      /* valid: no read is skewed; bad_values: reads whose sum of |v| reaches 2^63 */
  tbc_ledger_errors skewed;                               /* read numbers; worst = the greatest skew_count, ties the earliest */
  uint32_t n_candidates, reserved0;                       /* the reads the pair kernel took: n_partial + the complete reads skewed with a complete read */
  uint64_t n_checked;                                     /* read micro-ops checked */
  uint64_t n_pairs;                                       /* unordered skewed pairs */
  uint64_t ns_device;                                     /* the kernels, between HIP events */
  uint64_t bytes_in;                                      /* copied to the device */
} tbc_ledger_snap_summary;

typedef struct tbc_ledger_snap_out {      /* arrays caller-allocated, each optional (NULL = not wanted) */
  uint32_t *skew_count, *skew_first;      /* [n_ok_reads] */
  uint32_t* skew_key;                     /* [n_ok_reads][2] */
  uint8_t* snap_flags;                    /* [n_ok_reads] */
  tbc_ledger_snap_summary summary;
} tbc_ledger_snap_out;
tbc_status tbc_ledger_snapshots(const tbc_ledger_in* in, tbc_ledger_snap_out* out);

/* ------------------------------------------------------------------- ledger: the journal audit
 * An :ok :l-t lookup returns the ledger's JOURNAL: every transfer's id, debit-acct, credit-acct and amount.  tbc_ledger_check asks one
 * thing of it, and only of the final lookups (does it hold every invoked id).  This entry point audits EVERY :ok lookup, entry by
 * entry, against the transfers as they were invoked, against real time, and against the balances the reads returned.  THE RULES ARE
 * STATED ONCE, in the docstring of jepsen/ledger.py ("Journal audit"): records, lookups, entry_bits, present / repeated / failed /
 * early / lost / vanished, the books, reads ahead of and behind a lookup, the summary, the ranges.
 * Input: a tbc_ledger_rt_in, as tbc_ledger_realtime takes it (the columns, process, the inits, ok_transfers_apply).
 * Rows: transfer micro-ops are those of the ops with INVOKE && kind == TRANSFER, in column order; lookups are the ops with OK && kind ==
 * LOOKUP, final or not, in history order (tbc_ledger_check numbers only the final ones); entries are the lookups' micro-ops in column
 * order; reads are numbered as for tbc_ledger_check.
 *   entry_bits[e]        1 unknown, 2 altered
 *   lk_counts[l][k]      k = TBC_LEDGER_JN_*: entries (unknown, altered, repeated), records (failed, early, lost, vanished), reads
 *                        (ahead, behind)
 *   lk_present[l]        the records present in lookup l
 *   lk_vector[l][c]      the books of lookup l, c = 2 x (the account's position in `accounts`) + (0 credits-posted, 1 debits-posted)
 *   rd_bits[r]           1 ahead of some lookup, 2 behind some lookup;  rd_first[r][2]  the least lookup number of each, TBC_NO_OP
 *   xfer_present / early / lost / vanished[m]   per transfer micro-op, numbers of lookups; 0 for a reinvoked micro-op
 *   xfer_flags[m]        1 reinvoked, 2 nil
 * The host plans what is O(ops) (csrc/ledger_journal_plan.h) and reads no transfer or lookup micro-op; the device gets id, a, b, c and
 * flags of the transfer micro-ops and of the entries (33 bytes each) and id, a, b and flags of the reads' (25 bytes), and does the rest
 * (csrc/ledger_journal_kernels.h).  Every rule of tbc_ledger_realtime's input, and fewer than 2^31 transfer micro-ops, fewer than 2^31
 * entries a lookup, lookups x ceil(transfer micro-ops / 32) < 2^31 and reads x counters < 2^31: TBC_ERR_INVALID_ARG before any device
 * call, the message names the entry point and the op.  An amount of a non-nil record outside [0, 2^31) is counted ON THE DEVICE:
 * TBC_ERR_UNSUPPORTED, no results, summary.bad_amounts says how many.  No gfx950 device: TBC_ERR_NO_DEVICE (no CPU fallback).
 * One-shot and re-entrant as tbc_ledger_check is. */
enum { TBC_LEDGER_JN_UNKNOWN = 0, TBC_LEDGER_JN_ALTERED = 1, TBC_LEDGER_JN_REPEATED = 2, TBC_LEDGER_JN_FAILED = 3, TBC_LEDGER_JN_EARLY = 4,
       TBC_LEDGER_JN_LOST = 5, TBC_LEDGER_JN_VANISHED = 6, TBC_LEDGER_JN_AHEAD = 7, TBC_LEDGER_JN_BEHIND = 8, TBC_LEDGER_JN_KINDS = 9 };
#define TBC_LEDGER_JN_ENTRY_UNKNOWN 1u
#define TBC_LEDGER_JN_ENTRY_ALTERED 2u
#define TBC_LEDGER_JN_XFER_REINVOKED 1u
#define TBC_LEDGER_JN_XFER_NIL 2u
#define TBC_LEDGER_JN_READ_AHEAD 1u
#define TBC_LEDGER_JN_READ_BEHIND 2u

typedef struct tbc_ledger_journal_summary {
  uint32_t n_lookups, n_xfer_mops, n_records, n_reinvoked;
  uint32_t foreign_sides;                                 /* sides of the records that name no account (a nil record: both); skipped */
  uint32_t bad_amounts;                                   /* amounts of non-nil records outside [0, 2^31) */
  uint32_t read_count, valid;                             /* valid: every total is 0 */
  tbc_ledger_errors errors[TBC_LEDGER_JN_KINDS];          /* lookup numbers; worst = the greatest count, ties the earliest */
  uint64_t totals[TBC_LEDGER_JN_KINDS];                   /* lk_counts summed over the lookups */
  uint64_t n_entries;
  uint64_t n_checked;                                     /* read micro-ops checked */
  uint64_t ns_device;                                     /* the kernels, between HIP events */
  uint64_t bytes_in;                                      /* copied to the device */
} tbc_ledger_journal_summary;

typedef struct tbc_ledger_journal_out {   /* arrays caller-allocated, each optional (NULL = not wanted) */
  uint8_t* entry_bits;                    /* [n_entries] */
  uint32_t* lk_counts;                    /* [n_lookups][TBC_LEDGER_JN_KINDS] */
  uint32_t* lk_present;                   /* [n_lookups] */
  int64_t* lk_vector;                     /* [n_lookups][2 * n_accounts] */
  uint8_t* rd_bits;                       /* [n_ok_reads] */
  uint32_t* rd_first;                     /* [n_ok_reads][2] */
  uint32_t *xfer_present, *xfer_early, *xfer_lost, *xfer_vanished;   /* [n_xfer_mops] */
  uint8_t* xfer_flags;                    /* [n_xfer_mops] */
  tbc_ledger_journal_summary summary;
} tbc_ledger_journal_out;
tbc_status tbc_ledger_journal(const tbc_ledger_rt_in* in, tbc_ledger_journal_out* out);

/* ------------------------------------------------------------------- ledger: cycles through partial reads
 * tbc_ledger_snapshots plus the regressed bit of tbc_ledger_realtime are the whole cycle search over monotonic-key and realtime edges
 * only while every read is complete.  This entry point decides the graph itself, partial reads included: the strongly connected
 * components of the :ok reads under MONOTONIC edges (R -> R' when both check a counter and R is below R' on it) and REALTIME edges
 * (ret(R) < inv(R')).  THE RULES ARE STATED ONCE, in the docstring of jepsen/ledger.py ("Cycle search"): reads, counters, complete /
 * partial, inv and ret, the edges, clean and core reads, the summary, the ranges; the reduction the device computes is
 * cycles_dense_numpy there.
 * Input: a tbc_ledger_rt_in; pairing uses `process`; init_credits, init_debits and ok_transfers_apply are validated and not read.
 * Rows: reads are numbered as for tbc_ledger_check.
 *   scc[r]         the least read number of r's strongly connected component when it has two or more reads, TBC_NO_OP otherwise
 *   cyc_flags[r]   TBC_LEDGER_CYC_PARTIAL | TBC_LEDGER_CYC_ON_CYCLE | TBC_LEDGER_CYC_CORE
 * The host plans what is O(ops) (csrc/ledger_cycles_plan.h: the snapshot plan, and inv / ret by pairing).  The device repeats the
 * layout, sort and scan of tbc_ledger_snapshots, separates the CLEAN reads -- complete, comparable with every complete read, not
 * contradicted by real time: a chain of classes that is acyclic by itself -- from the CORE (every other read), describes each core read by
 * the classes it reaches and is reached from, builds the core's m x m bit matrix of direct and clean-mediated edges, closes it by
 * boolean squaring (summary.closure_rounds), and joins the clean reads to the components that enclose them
 * (csrc/ledger_cycles_kernels.h).  A history without core reads allocates no matrix and launches no closure or membership kernel.
 * Validation and errors are those of tbc_ledger_realtime's input and of tbc_ledger_snapshots: TBC_ERR_INVALID_ARG before any device
 * call; a read whose sum of |v| reaches 2^63 is counted on the device: TBC_ERR_UNSUPPORTED, no results, summary.bad_values.  A core of
 * more than TBC_LEDGER_CYCLES_MAX_CORE reads (two matrices of m^2 / 8 bytes: 64 MB at the cap): TBC_ERR_UNSUPPORTED with
 * summary.n_core (and read_count, n_partial) filled and no arrays.  One-shot and re-entrant as tbc_ledger_check is. */
#define TBC_LEDGER_CYCLES_MAX_CORE 16384u
#define TBC_LEDGER_CYC_PARTIAL  1u
#define TBC_LEDGER_CYC_ON_CYCLE 2u
#define TBC_LEDGER_CYC_CORE     4u

typedef struct tbc_ledger_cycles_summary {
  uint32_t read_count, n_partial, n_core, valid;          /* valid: no read is on a cycle */
  uint32_t n_on_cycle, n_components, first, largest;      /* first: the least read on a cycle; largest: the label of the largest component (ties the earliest); TBC_NO_OP */
  uint32_t largest_size, closure_rounds, bad_values, reserved0;   /* closure_rounds: squarings of the core's matrix, the one that changed nothing included */
  uint64_t n_checked;                                     /* read micro-ops checked */
  uint64_t ns_device;                                     /* the kernels, between HIP events */
  uint64_t bytes_in;                                      /* copied to the device */
} tbc_ledger_cycles_summary;

typedef struct tbc_ledger_cycles_out {    /* arrays caller-allocated, each optional (NULL = not wanted) */
  uint32_t* scc;                          /* [n_ok_reads] */
  uint8_t* cyc_flags;                     /* [n_ok_reads] */
  tbc_ledger_cycles_summary summary;
} tbc_ledger_cycles_out;
tbc_status tbc_ledger_cycles(const tbc_ledger_rt_in* in, tbc_ledger_cycles_out* out);

/* ------------------------------------------------------------------- perf: the series behind the reference's perf plots
 * checker/perf.clj composes latency-graph, rate-graph and open-ops-graph into every test.  What it PLOTS is out of scope (gnuplot,
 * ranges, nemesis shading); the SERIES it plots are computed here from op columns, decided on the device (csrc/perf_*.h;
 * jepsen/perf.py is the host statement and says every rule in full).  One row per op of the history, ALL ops, in history order:
 *   time     the op's :time in ns, 0 <= time < 2^52 (below that the reference's long(double(t) / 1e9) is t / 10^9 on integers)
 *   process  the client's :process; INT32_MIN where the op is not a client's (the nemesis): such an op enters t_max and nothing else
 *   type     TBC_PERF_T_*
 *   f        for a client op the number of its :f, numbered from 0 by first appearance among the client ops; n_f of them
 *   flags    TBC_PERF_F_CLIENT on exactly the ops whose process is not INT32_MIN
 * Pairing is the host plan's (knossos.history/pair-index: an invocation is completed by its process's next completion; a process's
 * second invocation leaves the first unmatched; a completion with nothing open is paired with nothing).  The OUTCOME of an
 * invocation is its completion's type (TBC_PERF_T_OK / FAIL / INFO), TBC_PERF_O_NONE if it has none; of a completion, its own type.
 *   t_max   = the greatest time of all ops, 0 if there is none;  nb_all = t_max / 10^9 + 1 one-second buckets;
 *   n_plot  = the buckets whose midpoint b + 0.5 is <= t_max / 1e9 compared as doubles (nb_all or nb_all - 1): the buckets plotted
 *   op_latency[i]     time[partner] - time[i] of a matched invocation, INT64_MIN for every other op
 *   op_outcome[i]     the outcome as above; TBC_PERF_O_NONE for an op that is not a client's
 *   op_open_after[i]  client ops with an outcome, per class (f, outcome): the running count in history order, +1 at an invocation,
 *                     -1 at a completion, as it stands after op i; 0 for every other op
 *   q_count[f][b]     the matched invocations of f whose OWN time is in bucket b (all outcomes together)
 *   q_value[f][b][j]  of their latencies in ascending order the one at min(n - 1, floor(n * q_j)), q = .5 .95 .99 1, n * q in
 *                     double; 0 where q_count is 0
 *   rate_count[f][o][b]  the client completions of f and type o + 1 (o = 0 OK, 1 FAIL, 2 INFO) whose own time is in bucket b
 *   open_last[f][o][b]   op_open_after of the LAST op in history order of class (f, o + 1) whose own time is in b; INT32_MIN: none
 *   open_fill[f][o][b]   b < n_plot: open_last carried forward over the buckets that have none, from 0
 * The caller sizes the arrays from tbc_perf_plan_sizes on the same input: the host plan alone, no device work.  n_f * 4 * nb_all
 * must stay below 2^31 (TBC_ERR_UNSUPPORTED).  A time out of range (an op without :time is passed as INT64_MIN) is
 * TBC_ERR_BAD_HISTORY; every other rule of the struct TBC_ERR_INVALID_ARG; the message names the entry point and the op.  Valid
 * input without a gfx950 device: TBC_ERR_NO_DEVICE (no CPU fallback).  One-shot and re-entrant as tbc_ledger_check is. */
enum { TBC_PERF_T_INVOKE = 0, TBC_PERF_T_OK = 1, TBC_PERF_T_FAIL = 2, TBC_PERF_T_INFO = 3 };
#define TBC_PERF_O_NONE   0u    /* op_outcome: none (otherwise a TBC_PERF_T_*) */
#define TBC_PERF_F_CLIENT 1u
#define TBC_PERF_NO_PROCESS INT32_MIN
#define TBC_PERF_QUANTILES 4u   /* .5 .95 .99 1 */
/* A (f, bucket) cell of at most this many latencies is sorted in LDS by one workgroup; a larger one takes the radix select. */
#define TBC_PERF_SELECT_TILE 2048u

typedef struct tbc_perf_in {
  uint32_t n_ops, device;
  const int64_t* time;
  const int32_t* process;
  const uint8_t *type, *flags;
  const uint16_t* f;
  uint32_t n_f, reserved0;
} tbc_perf_in;

typedef struct tbc_perf_sizes {
  uint32_t n_ops, n_f, nb_all, n_plot;
  int64_t t_max;
} tbc_perf_sizes;

typedef struct tbc_perf_summary {
  uint32_t n_ops, n_client, n_invocations, n_matched;   /* n_matched: invocations with a completion = latencies */
  uint32_t n_completions, n_f, nb_all, n_plot;          /* n_completions: client ops that are no invocation */
  uint32_t max_cell, reserved0;                         /* the greatest q_count */
  int64_t t_max;
  uint64_t ns_device;                                   /* the kernels, between HIP events */
  uint64_t bytes_in;                                    /* copied to the device */
} tbc_perf_summary;

typedef struct tbc_perf_out {             /* arrays caller-allocated, each optional (NULL = not wanted) */
  int64_t* op_latency;                    /* [n_ops] */
  uint8_t* op_outcome;                    /* [n_ops] */
  int32_t* op_open_after;                 /* [n_ops] */
  uint32_t* q_count;                      /* [n_f][nb_all] */
  int64_t* q_value;                       /* [n_f][nb_all][4] ns */
  uint32_t* rate_count;                   /* [n_f][3][nb_all] */
  int32_t* open_last;                     /* [n_f][3][nb_all] */
  int32_t* open_fill;                     /* [n_f][3][n_plot] */
  tbc_perf_summary summary;
} tbc_perf_out;
tbc_status tbc_perf_plan_sizes(const tbc_perf_in* in, tbc_perf_sizes* sizes);
tbc_status tbc_perf_series(const tbc_perf_in* in, tbc_perf_out* out);

/* ------------------------------------------------------------------- pairing on the device, many histories a call
 * tbc_pair_events_batch: tbc_pair_events for n_hist event histories at once, decided on the device (csrc/pair_*.h).  History h owns
 * the rows [ev_off[h], ev_off[h + 1]) of the five event columns, which are those of tbc_events concatenated; ev_off[0] = 0, ascending,
 * a history has fewer than 2^31 rows and a call 2^32 - 1 at most.  The columns are caller-owned (pageable or pinned) and go to the
 * device as they are, 14 B a row.
 * Of a WELL-FORMED history the six op columns, op_off[h + 1] - op_off[h] and n_process[h] are bit for bit what tbc_pair_events
 * writes for that history alone (inv_pos / ret_pos are rows within the history); n_events[h] = its rows.  op_off, n_events and
 * n_process are the three descriptor arrays of tbc_batch_desc and tbc_batch_input; `word` is TBC_WIRE_WORD(f, a8, b8, process) as
 * tbc_batch_reload encodes it, so the pointers of a mapped input slot can be passed here and tbc_batch_submit_input called after.
 * A MALFORMED history (an invocation while the process's op is open; an invocation after the process's :info; a completion without an
 * invocation; an unknown :type code) has status[h] = TBC_ERR_BAD_HISTORY and bad_row[h] = the row tbc_pair_events names, contributes
 * no op and n_process[h] = 0; the other histories are unaffected, the call returns TBC_OK and n_bad counts the histories whose status
 * is not TBC_OK.  status[h] = TBC_ERR_UNSUPPORTED (no op, n_process[h] = 0, bad_row 0xFFFFFFFF): more than TBC_PAIR_MAX_PROCESS
 * distinct :process values among the history's rows (counted in steps of 64 rows up to and including the step of the first malformed
 * row: there it takes precedence, past it the history is malformed), or -- only when `word` is asked for
 * -- a surviving op the wire format does not hold (f > 15; a value outside 0..254 that is not nil, b looked at for :cas only).
 * More surviving ops in the call than ops_cap: TBC_ERR_INVALID_ARG, the count in tbc_last_error(), no op array written.  A null
 * argument, ev_off that does not start at 0 or descends, too many rows: TBC_ERR_INVALID_ARG, decided before the device is looked
 * for; valid input without a gfx950 device: TBC_ERR_NO_DEVICE (no CPU fallback).  One-shot and re-entrant as tbc_ledger_check is. */
#define TBC_PAIR_MAX_PROCESS 4096u
#define TBC_PAIR_NO_ROW 0xFFFFFFFFu

typedef struct tbc_event_batch {
  uint32_t n_hist, device;
  const uint64_t* ev_off;        /* [n_hist + 1] */
  const uint8_t* type;           /* the columns of tbc_events, [ev_off[n_hist]] each */
  const int32_t* process;
  const uint8_t* f;
  const int32_t* a;
  const int32_t* b;
} tbc_event_batch;

typedef struct tbc_pair_out {    /* every array caller-allocated */
  uint64_t ops_cap;              /* ops the op arrays hold */
  uint64_t* op_off;              /* [n_hist + 1] */
  uint32_t* n_events;            /* [n_hist] */
  uint32_t* n_process;           /* [n_hist] */
  uint8_t* f;                    /* [ops_cap]; f, a, b, process: NULL = not wanted */
  int32_t* a;
  int32_t* b;
  int32_t* process;
  uint32_t* inv_pos;             /* [ops_cap] */
  uint32_t* ret_pos;             /* [ops_cap] */
  uint32_t* word;                /* [ops_cap], NULL = not wanted */
  int32_t* status;               /* [n_hist] a tbc_status */
  uint32_t* bad_row;             /* [n_hist] TBC_PAIR_NO_ROW: none */
  uint32_t n_bad, reserved0;
  uint64_t n_ops;                /* = op_off[n_hist] */
  uint64_t ns_device;            /* the kernels, between HIP events */
  uint64_t bytes_in;             /* copied to the device */
} tbc_pair_out;
tbc_status tbc_pair_events_batch(const tbc_event_batch* in, tbc_pair_out* out);

/* ------------------------------------------------------------------- packed events, and events straight into a batch
 * THE PACKED EVENT WORD.  A batch takes what the wire format holds (f <= 15, values 0..254 or nil), so an event bound for one loses
 * nothing as TWO columns, 8 B a row instead of 14: a uint32_t ev_word and the int32_t process column as it is (process ids are
 * arbitrary and stay whole).  ev_word = TBC_EVENT_WORD(type, f, a, b) over ENCODED fields:
 *   bits 0-2    type   TBC_INVOKE .. TBC_INFO; TBC_EVW_TYPE_UNKNOWN (7) = a :type code that is none of them
 *   bits 3-7    f      0..15; TBC_EVW_F_ABOVE (16) = an :f above 15
 *   bits 8-16   a      0..254; TBC_EVW_NIL (255) = nil; TBC_EVW_UNFIT (256) = a value the wire format does not hold
 *   bits 17-25  b      as a
 * The three codes beside the values keep every rule of tbc_pair_events_batch with `word` asked for decidable from the packed form,
 * with the same answer: the malformed row (an unknown :type), and TBC_ERR_UNSUPPORTED for a SURVIVING op whose f, a -- or b of a
 * :cas -- does not fit (a failed op with such a value is still fine).  Read back, an encoded field is its value, the codes 7, 16
 * and 256 themselves, and TBC_EVW_NIL is TBC_NIL.
 * tbc_pack_events: one history's five columns -> its words, ev_word[ev->n]; host code, no device (the process column is not touched:
 * the caller passes it on beside the words).
 * tbc_pair_packed_batch: tbc_pair_events_batch over the packed form -- the same plan, kernels, steps and output contract, the events
 * those the words decode to; it differs in what is copied in: bytes_in = 8 B a row + 8 B * (n_hist + 1). */
#define TBC_EVW_TYPE_UNKNOWN 7u
#define TBC_EVW_F_ABOVE 16u
#define TBC_EVW_NIL 255u
#define TBC_EVW_UNFIT 256u
#define TBC_EVENT_WORD(type, f, a, b) ((uint32_t)(type) | ((uint32_t)(f) << 3) | ((uint32_t)(a) << 8) | ((uint32_t)(b) << 17))
#define TBC_EVW_TYPE(w) ((uint32_t)(w) & 7u)
#define TBC_EVW_F(w) (((uint32_t)(w) >> 3) & 31u)
#define TBC_EVW_A(w) (((uint32_t)(w) >> 8) & 511u)
#define TBC_EVW_B(w) (((uint32_t)(w) >> 17) & 511u)
#define TBC_EVW_VALUE(v9) ((v9) == TBC_EVW_NIL ? TBC_NIL : (int32_t)(v9))      /* an encoded a / b read back */

tbc_status tbc_pack_events(const tbc_events* ev, uint32_t* ev_word);

typedef struct tbc_packed_event_batch {
  uint32_t n_hist, device;
  const uint64_t* ev_off;        /* [n_hist + 1] as tbc_event_batch.ev_off */
  const uint32_t* ev_word;       /* [ev_off[n_hist]] */
  const int32_t* process;        /* [ev_off[n_hist]] */
} tbc_packed_event_batch;
tbc_status tbc_pair_packed_batch(const tbc_packed_event_batch* in, tbc_pair_out* out);

/* EVENTS INTO A BATCH.  tbc_batch_map_events / tbc_batch_submit_events are to event histories what tbc_batch_map_input /
 * tbc_batch_submit_input are to op columns: the caller writes packed events into library-owned PINNED memory, the library pairs them
 * on the device (the kernels of tbc_pair_events_batch, on the batch's COPY stream, so under whatever the batch is searching) and the
 * wire columns are emitted straight into the batch's device stage; only the per-history descriptors come back.
 *   tbc_batch_map_events     the event slots (slot < 16) are a second set of pinned slots, apart from the op slots.  events_cap = 0
 *                            means 3 * the batch's ops_cap (tbc_input_info); the FIRST mapping fixes events_cap for the batch and a
 *                            later, larger request is TBC_ERR_INVALID_ARG.  Waits until the slot's previous events have left for the
 *                            device.  The first mapping also allocates the batch's device event arena, once, kept until
 *                            tbc_batch_destroy (24 B an event and 36 B a history; tbc_batch_device_bytes counts it).
 *   tbc_batch_submit_events  the slot holds n_hist histories: ev_off[0..n_hist] (the rules of tbc_event_batch.ev_off), the words, the
 *                            process column.  Validated on the host in O(histories) (INVALID_ARG: ev_off; n_hist = 0 or beyond the
 *                            batch's n_hist_cap; more events than events_cap; two inputs pending already; the slot unmapped or still
 *                            being copied).  Then the three arrays go up, the histories are paired, and the descriptors -- op_off,
 *                            n_events, n_process, status, bad_row, the totals: TBC_EVENTS_DESC_BYTES(n_hist) -- come back; the call
 *                            BLOCKS its thread until the pairing is done (it never waits for the compute stream) and fills `rep`
 *                            (null: no report).  ALL OR NOTHING: a history that is not TBC_OK -> TBC_ERR_BAD_HISTORY if one is
 *                            malformed, else TBC_ERR_UNSUPPORTED; more surviving ops than the batch's ops_cap -> TBC_ERR_INVALID_ARG,
 *                            the count in tbc_last_error().  Then nothing is pending, no stage has been written and the batch still
 *                            answers its resident input.  Otherwise the input is laid out as tbc_batch_submit_input lays one out
 *                            (the same refusals), its wire columns are emitted into the stage and it is pending: the next
 *                            tbc_batch_run consumes it.
 * tbc_input_info.bytes_copied of such an input is what crossed PCIe for it: 8 B an event + 8 B * (n_hist + 1) up and
 * TBC_EVENTS_DESC_BYTES(n_hist) down (an op input: 12 B an op).
 * A COUNT-FORM batch plans its crashed calls on the host from the wire words, which this route never brings to the host:
 * tbc_batch_submit_events on one is TBC_ERR_UNSUPPORTED; its route is tbc_pair_events_batch into a mapped OP slot and
 * tbc_batch_submit_input.  Batches that take no fresh inputs refuse as tbc_batch_map_input refuses. */
#define TBC_EVENTS_DESC_BYTES(n_hist) (16ull + 8ull * ((uint64_t)(n_hist) + 1ull) + 16ull * (uint64_t)(n_hist))

typedef struct tbc_batch_events {  /* pointers into one pinned slot; valid until the batch is destroyed */
  uint32_t n_hist_cap, reserved0;
  uint64_t events_cap;
  uint64_t* ev_off;                /* [n_hist_cap + 1] */
  uint32_t* ev_word;               /* [events_cap] */
  int32_t* process;                /* [events_cap] */
} tbc_batch_events;

typedef struct tbc_events_report { /* arrays caller-allocated, [n_hist]; each optional */
  int32_t* status;                 /* a tbc_status per history */
  uint32_t* bad_row;               /* TBC_PAIR_NO_ROW: none */
  uint32_t n_bad, reserved0;
  uint64_t n_ops;                  /* surviving ops of the input */
  uint64_t ns_device;              /* the pairing kernels, between HIP events */
  uint64_t bytes_in;               /* copied to the device */
} tbc_events_report;

tbc_status tbc_batch_map_events(tbc_batch* b, uint32_t slot, uint64_t events_cap, tbc_batch_events* out);
tbc_status tbc_batch_submit_events(tbc_batch* b, uint32_t slot, uint32_t n_hist, tbc_events_report* rep);

/* ------------------------------------------------------------------- one keyed history, split by key on the device
 * A run under jepsen.independent leaves ONE event history whose values are [k v] tuples; the histories per key exist only after
 * independent/subhistory.  tbc_pair_keyed_events takes that one history as it is -- the event columns (packed: ev_word + process,
 * 8 B a row; or the five columns, 14 B) beside a key column, 4 B a row -- splits it by key on the device (csrc/split_*.h) and pairs
 * every key's rows (the kernels of tbc_pair_events_batch, unchanged) in the same call; nothing returns to the host in between but the
 * number of keys.  Rows that belong to every key (nemesis ops, values that are no tuple) are no client op of any key's object: the
 * caller leaves them out.
 *   keys[0 .. n_keys)       the distinct keys in order of FIRST APPEARANCE (every int32_t is a key)
 *   ev_off[k], ev_off[k+1]  key k's rows in the split order; within a key the rows keep the order they had (a stable split)
 *   row_of[j]               the original row of split row j (NULL: not wanted)
 *   out                     the contract of tbc_pair_events_batch over n_keys histories, history h = keys[h]; inv_pos / ret_pos are rows
 *                           within the key's rows; a malformed or unsupported key costs its own status[h].  NULL: split only.
 * More distinct keys than keys_cap: TBC_ERR_INVALID_ARG, the count in tbc_last_error(), nothing written (decided before the rows are
 * sorted); more surviving ops than out->ops_cap: as tbc_pair_events_batch, and the split is not written either.  Null arguments
 * and more than 2^32 - 2 rows: TBC_ERR_INVALID_ARG before the device is looked for; valid input without a gfx950 device:
 * TBC_ERR_NO_DEVICE.  n = 0: TBC_OK, n_keys = 0, ev_off[0] = 0.  out->bytes_in counts 12 B a row packed, 18 B in columns. */
typedef struct tbc_keyed_events {      /* ONE history; ev_word non-null: the packed form, else the five columns */
  uint32_t n, device;
  const int32_t* key;                  /* [n] */
  const uint32_t* ev_word; const int32_t* process;
  const uint8_t* type; const uint8_t* f; const int32_t* a; const int32_t* b;
} tbc_keyed_events;
typedef struct tbc_split_out {         /* caller-allocated */
  uint32_t keys_cap, n_keys;
  int32_t* keys;                       /* [keys_cap] */
  uint64_t* ev_off;                    /* [keys_cap + 1] */
  uint32_t* row_of;                    /* [n], NULL = not wanted */
} tbc_split_out;
tbc_status tbc_pair_keyed_events(const tbc_keyed_events* in, tbc_split_out* split, tbc_pair_out* out);

/* ONE KEYED HISTORY INTO A BATCH.  tbc_batch_map_keyed_events / tbc_batch_submit_keyed_events are tbc_batch_map_events /
 * tbc_batch_submit_events with the split in front: the caller writes ONE history -- a key, a packed word and a process per event,
 * 12 B -- into a pinned event slot; on the batch's copy stream the events are split by key (the kernels of tbc_pair_keyed_events), the
 * gather writes where tbc_batch_submit_events' copies land, and from there on the call IS tbc_batch_submit_events: the keys' histories
 * are paired, the descriptors come back, and -- all or nothing, the same refusals -- the wire columns are emitted into the device
 * stage.  History h of the input is key keys[h].
 *   tbc_batch_map_keyed_events     the event slots of tbc_batch_map_events (the key array lies in the same pinned allocation); the
 *                                  first mapping of either kind fixes events_cap.  The first KEYED mapping adds the split's regions
 *                                  to the batch's device memory, once (tbc_batch_device_bytes counts them): the raw input, the key
 *                                  table, ids and the sort's scratch, about 60 to 80 B an event.
 *   tbc_batch_submit_keyed_events  n_events rows of the slot.  TBC_ERR_INVALID_ARG, nothing pending and no stage written: n_events = 0
 *                                  or beyond events_cap; more distinct keys than the batch's n_hist_cap (the count in
 *                                  tbc_last_error(), decided before a row moves: rep then holds n_keys, bytes_in, the kernels so far
 *                                  in ns_device, and zeros); and what tbc_batch_submit_events refuses.  rep
 *                                  (null: none): tbc_events_report's fields, n_keys, and -- each optional -- keys[n_hist_cap] and
 *                                  row_of[n_events] (4 B an event back only when asked for).  ns_device: the split's and the
 *                                  pairing's kernels; bytes_in: 12 B an event.
 * A count-form batch refuses as it refuses tbc_batch_submit_events. */
typedef struct tbc_batch_keyed_events { /* pointers into one pinned slot; valid until the batch is destroyed */
  uint32_t n_hist_cap, reserved0;
  uint64_t events_cap;
  int32_t* key;                    /* [events_cap] */
  uint32_t* ev_word;               /* [events_cap] */
  int32_t* process;                /* [events_cap] */
} tbc_batch_keyed_events;

typedef struct tbc_keyed_report {  /* arrays caller-allocated; each optional */
  int32_t* status;                 /* [n_hist_cap] a tbc_status per key */
  uint32_t* bad_row;               /* [n_hist_cap] a row within the key's rows; TBC_PAIR_NO_ROW: none */
  uint32_t n_bad, reserved0;
  uint64_t n_ops;
  uint64_t ns_device;
  uint64_t bytes_in;
  uint32_t n_keys, reserved1;
  int32_t* keys;                   /* [n_hist_cap] in order of first appearance */
  uint32_t* row_of;                /* [n_events] the original row of every split row */
} tbc_keyed_report;

tbc_status tbc_batch_map_keyed_events(tbc_batch* b, uint32_t slot, uint64_t events_cap, tbc_batch_keyed_events* out);
tbc_status tbc_batch_submit_keyed_events(tbc_batch* b, uint32_t slot, uint64_t n_events, tbc_keyed_report* rep);

/* ------------------------------------------------------------------- misc */
uint32_t tbc_version(void);             /* TBC_ABI_VERSION                       */
const char* tbc_strerror(int status);
const char* tbc_last_error(void);       /* thread-local detail of the last error */
int32_t tbc_device_count(void);         /* gfx950 devices visible; 0 if none     */
/* diagnostics: with TBC_DEBUG=1 in the environment the kernels mirror their progress into
 * host-mapped words; this copies up to n (<= 64) of them.  Returns 0 when disabled. */
int tbc_debug_peek(uint32_t* out, uint32_t n);
/* Environment switches, read at launch time -- for experiments and A/B tests, never needed for correct results:
 *   TBC_OPEN_WALK=slots           build the per-front tables with lane = process slot for batches of <= 64
 *                                 slots too (default: lane = front, open_walk_impl.h); same tables either way
 *   TBC_NARROW_WAVES_PER_SIMD=n   wavefronts per SIMD the several-histories-per-wavefront search is launched at
 *                                 (default 4, the build's maximum)
 *   TBC_SWEEP=0|1, TBC_SWEEP_SEG=n  never / whenever possible take the level sweep; its segment length
 *   TBC_SWEEP_WG=0|4|8            wavefronts per segment of a sweep of at most 4,096 wavefronts (default 8: a workgroup per segment,
 *                                 jit_sweep_wg.hip; 0 = one wavefront per segment always)
 *   TBC_SWEEP_WG_RING=1           (experimental) the workgroup sweep gathers a sub-round's children in a ring before inserting them
 *   TBC_SWEEP_WG_FP=1             (experimental) ... keeps 8 bits of a key's hash in its table word (a probe past another key reads no key)
 *   TBC_SWEEP_WG_COMPACT=1|2      (experimental) ... a wide sub-round numbers its children first and inserts 512 CHILDREN a pass (not with the ring);
 *                                 2 = and a pass that fits one wavefront is run by wavefront 0 alone
 *   TBC_NARROW_LEAN=1|2           (experimental; 2 = and the lookahead at once only for the config that is popped next) several histories per wavefront over lean tables: a list entry {call, twin mask} in one array,
 *                                 an 8 B lookahead record (two producer slots; three or more read as "one is still to be linearized")
 *   TBC_NARROW_ORDER=1|2|16+W     (experimental) ... with every front's list in order of completion: the call that completes soonest is tried
 *                                 first (fewer rounds for the same probes); a witness's absorbed reads follow the same order;
 *                                 2 = and the :write calls after everything else (a :cas the state allows now before a :write);
 *                                 16 + W = and a :write as if it completed W ranks later (the soft form of 2; W = 16 .. 24)
 *   TBC_PACK_ONE=1|2              (experimental) a handful of histories are packed by sixteen wavefronts each, tables in LDS (pack_one.hip);
 *                                 2 = and the per-front counts in the same launch
 *   TBC_PACK_WG=1                 (experimental) a batch of the wide schedule is packed by four wavefronts per history, tables in LDS,
 *                                 and the same pass leaves the per-front counts (pack_one.hip, pack_wg_kernel); 2 = a batch that
 *                                 cannot take it is TBC_ERR_UNSUPPORTED instead of silently the default kernels
 *   TBC_DEBUG=1, TBC_SYNC_EACH=1  progress words (above), a traced synchronisation after every launch */

#ifdef __cplusplus
}
#endif
#endif /* TBCHECK_H */
