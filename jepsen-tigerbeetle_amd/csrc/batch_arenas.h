// batch_arenas.h -- the device arenas of a batch whose size follows the RESIDENT INPUT, each stated once with its element count.
// tbc_batch_create visits them to allocate (batch_create.hip, alloc_arenas), a fresh input that has outgrown the batch visits them to
// replace what is too small (batch_stream.hip, ensure_arenas).  An arena of this kind is added HERE (and declared in tbc_batch.h); it
// frees itself (DevBuf).
//
// A count comes from the batch's decisions (lanes, rules, vpad, mask_words, lookahead, count_form, any_crashed, opts.want_witness),
// the layout's totals and a number of histories `nh` (create: the batch's; a fresh input: what a slot holds, in_hist_cap).  A count
// of 0 is an arena of one element nobody reads: it exists, so that a kernel's argument is never null, and it never grows.
//
// THE ORDER is tbc_batch_create's allocation order, in three runs with what is not the input's between them -- tbc_check's arenas are
// consecutive pieces of its context's slab, and two of its fast paths hold only while
//   visit_column_arenas   d_f .. d_ret, followed by d_hist, d_bh, d_work, go up as one block (batch_create.hip, upload_inputs)
//   visit_zeroed_arenas   d_bitmap, d_off, d_ncr, followed by d_pool_cursor, are zeroed by one memset (batch_run.hip, first_pass)
//   visit_other_arenas    everything else, in any order
// What is NOT here: arenas of `nh` entries (d_hist, d_bh, d_work, d_results, d_cfg, d_park: a fresh input never has more histories than
// in_hist_cap), the sweeps' arenas (such a batch takes no fresh input), d_queue, d_pool_vals, d_table, the progress words; the lists
// (size_lists below: they are sized by entries, on the device or after a run) and the growth pool (pool_share_words: create and a
// fresh input take their share by rules of their own).
#pragma once
#include "tbc_batch.h"

namespace tbc {

// u64 words of the batch's own visited-set arena
inline uint64_t btab_words(const tbc_batch* B, const LayoutTotals& t) { return t.btab_n * B->tab_stride(); }

// The growth pool's share of the visited-set arena: 30 % -- 10 % for the big quiet batches that run several histories per wavefront,
// whose sets rarely grow (a history that outgrows its table and finds the pool empty is run again from a scratch arena: at 32 calls in
// flight a 10 % pool cost 22 s of such retries per 2,048 histories) --, at most 32 GiB
inline uint64_t pool_share_words(const tbc_batch* B, const LayoutTotals& t) {
  return std::min<uint64_t>(btab_words(B, t) * (B->lanes ? 1u : 3u) / 10, (32ull << 30) / 8);
}

// v(arena, elements) -> tbc_status; the first status that is not TBC_OK ends the visit
template <typename V>
tbc_status visit_column_arenas(tbc_batch* B, const LayoutTotals& t, V&& v) {
  const uint64_t T = t.total_ops;
  tbc_status s;
  if ((s = v(B->d_f, T)) || (s = v(B->d_a, T)) || (s = v(B->d_b, T)) || (s = v(B->d_proc, T)) || (s = v(B->d_inv, T)) || (s = v(B->d_ret, T))) return s;
  return TBC_OK;
}

template <typename V>
tbc_status visit_zeroed_arenas(tbc_batch* B, const LayoutTotals& t, V&& v) {
  const uint64_t fronts = B->width > 1 ? t.boff_n : 0;
  tbc_status s;
  if ((s = v(B->d_bitmap, t.bm_n)) || (s = v(B->d_off, fronts)) || (s = v(B->d_ncr, fronts))) return s;
  return TBC_OK;
}

template <typename V>
tbc_status visit_other_arenas(tbc_batch* B, const LayoutTotals& t, uint32_t nh, V&& v) {
  const uint64_t T = t.total_ops;
  const uint32_t MW = B->mask_words;
  tbc_status s;
  if ((s = v(B->d_rec, t.rec_n)) || (s = v(B->d_seg, t.seg_n)) || (s = v(B->d_ret_slot, T)) || (s = v(B->d_ret_op, T)) ||
      (s = v(B->d_wpre, t.bm_n)) || (s = v(B->d_frames, t.frame_n)) || (s = v(B->d_tab, t.tab_n)) ||
      (s = v(B->d_witness, B->opts.want_witness ? T : 0)))
    return s;
  if (B->width <= 1) return TBC_OK;
  // ---- the wide schedule's
  if ((s = v(B->d_crashed, (B->count_form || !B->any_crashed) ? 0 : T)) || (s = v(B->d_cmem, B->count_form ? t.bocc_n : 0)) ||
      (s = v(B->d_slot8, slot8_bytes(T, nh))) || (s = v(B->d_stack, t.bstack_n)) || (s = v(B->d_btab, btab_words(B, t))))
    return s;
  if (B->lanes && (s = v(B->d_rk8, slot8_bytes(T, nh)))) return s;
  // several histories per wavefront: front records (tbc_internal.h) instead of plain rows, with or without the rules
  if (B->lanes) { if ((s = v(B->d_rdm, T * B->front_words()))) return s; }
  else if (B->reg_rules() && (s = v(B->d_rdm, T * B->vpad * MW))) return s;
  // (d_looktmp: scratch of the walk with lane = process slot only)
  if (B->lookahead && ((s = v(B->d_look, look_words(T, nh, MW))) || (s = v(B->d_looktmp, walk_by_front(MW, B->vpad) ? 0 : T)) ||
                       (s = v(B->d_dstack, t.bstack_n))))
    return s;
  return TBC_OK;
}

template <typename V>
tbc_status visit_input_arenas(tbc_batch* B, const LayoutTotals& t, uint32_t nh, V&& v) {
  tbc_status s;
  if ((s = visit_column_arenas(B, t, v)) || (s = visit_zeroed_arenas(B, t, v)) || (s = visit_other_arenas(B, t, nh, v))) return s;
  return TBC_OK;
}

// ---- the per-front lists of open calls: d_lst, and under the register family's rules a twin word per mask word of every entry (d_twn)

// the narrow kernel addresses the lists with 32-bit element offsets (wgl_narrow_impl.h): that many entries are beyond several histories
// per wavefront.  What follows is the caller's: skip, refuse, keep a fallback, drop to a wavefront per history.
inline bool lists_past_lanes(const tbc_batch* B, uint64_t entries) { return B->lanes && entries >= (1ull << 32); }

// both arenas for `entries` entries; what they held is gone
inline tbc_status size_lists(tbc_batch* B, uint64_t entries) {
  tbc_status s;
  if ((s = B->d_lst.regrow((size_t)entries))) return s;
  return B->reg_rules() ? B->d_twn.regrow((size_t)(entries * B->mask_words)) : TBC_OK;
}

}  // namespace tbc
