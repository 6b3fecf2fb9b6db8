// omf_plan_layout.cpp — the QSGD plan's work-item tables and encoder choice (host only).
#include "omf_plan_layout.h"

#include <algorithm>
#include <utility>

namespace omf {
namespace plan_layout {

namespace {

// Ticket-order item sequence.  Register-resident tensors (<= cap items of ev * 1024) are
// emitted in place; a larger tensor emits its NORM items in place and its QUANT items
// after the next tensor's items (one tensor of slack for the norm hand-off).
void build_sequence(const Desc& d, bool resident_ok, std::vector<Item>& seq, std::vector<TensorInfo>& tinfo,
                    int64_t& npart) {
  seq.clear();
  tinfo.assign(d.nt, TensorInfo{});
  npart = 0;
  std::vector<Item> deferred;
  for (int32_t t = 0; t < d.nt; ++t) {
    const int64_t n = d.sizes[t], b = d.offsets[t];
    const int64_t es = (int64_t)d.ev * 1024;
    const int64_t ns = (n + es - 1) / es;
    std::vector<Item> q_t;
    if (ns == 1 || (resident_ok && ns <= d.cap)) {
      tinfo[t] = TensorInfo{b, n, es, (int32_t)ns, (int32_t)npart};
      for (int64_t c = 0; c < ns; ++c) {
        const int64_t cb = b + c * es;
        seq.push_back(Item{cb, std::min(b + n, cb + es), t, kResident, (int32_t)c, 0});
      }
      npart += ns;
    } else {
      const int64_t nc = (n + d.chunk - 1) / d.chunk;
      tinfo[t] = TensorInfo{b, n, d.chunk, (int32_t)nc, (int32_t)npart};
      for (int64_t c = 0; c < nc; ++c) {
        const int64_t cb = b + c * d.chunk, ce = std::min(b + n, cb + d.chunk);
        seq.push_back(Item{cb, ce, t, kNorm, (int32_t)c, 0});
        q_t.push_back(Item{cb, ce, t, kQuant, (int32_t)c, 0});
      }
      npart += nc;
    }
    seq.insert(seq.end(), deferred.begin(), deferred.end());
    deferred.swap(q_t);
  }
  seq.insert(seq.end(), deferred.begin(), deferred.end());
}

// Register-resident ring encoder (omf_qsgd_ring.hip qsgd_encode_rr): every single-read tensor
// lies inside one row of `grid` consecutive items, so all its chunks are at the same
// position of their workgroups.  Rows are packed first-fit decreasing; gaps are filled
// with NORM items of the multi-row ("big") tensors, or with empty items when none are
// left.  Layout: [whole rows of big NORM items][packed rows][remaining big NORM items]
// [big QUANT items] — every NORM item precedes its tensor's QUANT items.
void build_rr_sequence(const Desc& d, Tables& o) {
  namespace R = omf::ring;
  const int64_t ch = d.ring_chunk;
  const int64_t G = std::max<int32_t>(d.ring_grid, 1);
  o.ring_hold_max = d.ring_hold_override > 0 ? std::min<int64_t>(G, d.ring_hold_override) : G;
  std::vector<R::Item>& seq = o.ring;
  std::vector<R::Tensor>& tens = o.ring_t;
  seq.clear();
  tens.assign(d.nt, R::Tensor{});
  std::vector<R::Item> norm_items, quant_items;
  std::vector<std::pair<int64_t, int32_t>> regular;  // (chunks, tensor)
  int64_t gb = 0;
  o.ring_two_pass = 0;
  auto item = [&](int32_t t, int64_t k, int32_t flags) {
    const int64_t n = d.sizes[t], b = d.offsets[t], cb = b + k * ch;
    return R::Item{cb, std::min(b + n, cb + ch), b, n, t, flags, (int32_t)k, tens[t].nchunks, tens[t].gbase, {0, 0, 0}};
  };
  for (int32_t t = 0; t < d.nt; ++t) {
    const int64_t nc = (d.sizes[t] + ch - 1) / ch;
    tens[t] = R::Tensor{d.offsets[t], d.sizes[t], (int32_t)nc, (int32_t)gb, {0, 0}};
    gb += nc;
    if (nc <= o.ring_hold_max) {
      regular.emplace_back(nc, t);
    } else {
      ++o.ring_two_pass;
      for (int64_t k = 0; k < nc; ++k) norm_items.push_back(item(t, k, R::kPublish));
      for (int64_t k = 0; k < nc; ++k) quant_items.push_back(item(t, k, R::kQuant));
    }
  }
  std::stable_sort(regular.begin(), regular.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
  std::vector<std::vector<int32_t>> rows;
  std::vector<int64_t> room;
  for (const auto& r : regular) {
    size_t i = 0;
    while (i < rows.size() && room[i] < r.first) ++i;
    if (i == rows.size()) {
      rows.emplace_back();
      room.push_back(G);
    }
    rows[i].push_back(r.second);
    room[i] -= r.first;
  }
  // Gap fillers come from the back of the NORM list; whole rows of the rest lead.
  size_t nfill = 0;
  for (size_t i = 0; i + 1 < rows.size(); ++i) nfill += (size_t)room[i];
  nfill = std::min(nfill, norm_items.size());
  const size_t avail = norm_items.size() - nfill;
  const size_t lead = avail / (size_t)G * (size_t)G;
  seq.insert(seq.end(), norm_items.begin(), norm_items.begin() + (ptrdiff_t)lead);
  size_t tail = lead;                           // next NORM item not yet placed (after the lead rows)
  size_t fill = norm_items.size() - nfill;      // next gap filler
  for (size_t i = 0; i < rows.size(); ++i) {
    for (int32_t t : rows[i])
      for (int64_t k = 0; k < tens[t].nchunks; ++k) seq.push_back(item(t, k, R::kPublish | R::kQuant));
    if (i + 1 < rows.size()) {
      for (int64_t g = 0; g < room[i]; ++g) {
        if (fill < norm_items.size()) seq.push_back(norm_items[fill++]);
        else seq.push_back(R::Item{0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}});  // empty: keeps rows aligned
      }
    }
  }
  seq.insert(seq.end(), norm_items.begin() + (ptrdiff_t)tail, norm_items.begin() + (ptrdiff_t)(norm_items.size() - nfill));
  seq.insert(seq.end(), quant_items.begin(), quant_items.end());
  o.n_ring_gran = std::max<int64_t>(gb, 1);
}

// Ring sequence: tensors of <= ring_hold_max chunks are HOLD chunks (read once);
// larger ones are NORM chunks (partial only) plus QUANT chunks (second read), the QUANT
// chunks placed ring_gap items later (big_mode 0) or at the very end with every NORM
// chunk first (big_mode 1).  Items are dealt to workgroups round-robin.
void build_ring_sequence(const Desc& d, Tables& o) {
  namespace R = omf::ring;
  if (d.ring_kind == 1) return build_rr_sequence(d, o);
  const int64_t ch = d.ring_chunk;
  o.ring_hold_max = d.ring_hold_override > 0 ? d.ring_hold_override : (int64_t)d.ring_slots * d.ring_grid;
  const int64_t gap = d.ring_gap >= 0 ? d.ring_gap : d.ring_grid;
  std::vector<R::Item>& seq = o.ring;
  std::vector<R::Tensor>& tens = o.ring_t;
  seq.clear();
  tens.assign(d.nt, R::Tensor{});
  std::vector<R::Item> front, back;
  std::vector<std::pair<int64_t, std::vector<R::Item>>> pending;  // (insert when seq.size() >= first, items)
  int64_t gb = 0;
  o.ring_two_pass = 0;
  auto flush = [&](bool all) {
    for (size_t i = 0; i < pending.size();) {
      if (all || (int64_t)seq.size() >= pending[i].first) {
        seq.insert(seq.end(), pending[i].second.begin(), pending[i].second.end());
        pending.erase(pending.begin() + i);
      } else {
        ++i;
      }
    }
  };
  for (int32_t t = 0; t < d.nt; ++t) {
    const int64_t n = d.sizes[t], b = d.offsets[t];
    const int64_t nc = (n + ch - 1) / ch;
    tens[t] = R::Tensor{b, n, (int32_t)nc, (int32_t)gb, {0, 0}};
    gb += nc;
    const bool big = nc > o.ring_hold_max;
    std::vector<R::Item> quant;
    for (int64_t k = 0; k < nc; ++k) {
      const int64_t cb = b + k * ch, ce = std::min(b + n, cb + ch);
      if (!big) {
        seq.push_back(R::Item{cb, ce, b, n, t, R::kPublish | R::kQuant, (int32_t)k, (int32_t)nc, (int32_t)(gb - nc), {0, 0, 0}});
        flush(false);
      } else {
        const R::Item norm_it{cb, ce, b, n, t, R::kPublish, (int32_t)k, (int32_t)nc, (int32_t)(gb - nc), {0, 0, 0}};
        if (d.ring_big_mode == 1) front.push_back(norm_it);
        else seq.push_back(norm_it);
        quant.push_back(R::Item{cb, ce, b, n, t, R::kQuant, (int32_t)k, (int32_t)nc, (int32_t)(gb - nc), {0, 0, 0}});
      }
    }
    if (big) {
      ++o.ring_two_pass;
      if (d.ring_big_mode == 1) back.insert(back.end(), quant.begin(), quant.end());
      else pending.emplace_back((int64_t)seq.size() + gap, std::move(quant));
    }
  }
  flush(true);
  if (d.ring_big_mode == 1) {
    seq.insert(seq.begin(), front.begin(), front.end());
    seq.insert(seq.end(), back.begin(), back.end());
  }
  o.n_ring_gran = std::max<int64_t>(gb, 1);
}

// Flat items (decode, norm-supplied quantise, Top-K passes): one 16 Ki sub-chunk each, the
// fastest decode granularity measured (profiles/r01_notes.md).  Bracketed encoder tables: one
// bracket item per tensor (one workgroup writes its bracket) and fold segments of kSpecSeg wave
// partials (kBlkWaves per 4 Ki block, kSub / kSpecBlk = 4 blocks per flat item).
void build_flat_tables(const Desc& d, Tables& o) {
  constexpr int64_t kItemParts = kBlkWaves * (kSub / kSpecBlk);  // wave partials per flat item
  o.flat.clear();
  o.br_items.clear();
  o.fold_items.clear();
  o.grid_pbeg.assign((size_t)d.nt, 0u);
  o.grid_pcnt.assign((size_t)d.nt, 0u);
  int32_t seg_base = 0;
  for (int32_t t = 0; t < d.nt; ++t) {
    const int64_t n = d.sizes[t], b = d.offsets[t];
    const int64_t p_begin = kItemParts * (int64_t)o.flat.size();
    for (int64_t c = 0; c * kSub < n; ++c) {
      const int64_t cb = b + c * kSub;
      o.flat.push_back(Item{cb, std::min(b + n, cb + kSub), t, kQuant, (int32_t)c, 0});
    }
    const int64_t p_end = kItemParts * (int64_t)o.flat.size();
    o.grid_pbeg[(size_t)t] = (uint32_t)(p_begin / kItemParts);  // the grid encoder: one partial per item
    o.grid_pcnt[(size_t)t] = (uint32_t)((p_end - p_begin) / kItemParts);
    const int64_t R = std::max<int64_t>(1, std::min<int64_t>(kSpecRuns, n / (2 * kSpecRun)));
    const int64_t Rw = std::max<int64_t>(1, std::min<int64_t>(kSpecRunsWide, n / (2 * kSpecRunWide)));
    o.br_items.push_back(SpecBrItem{b, n, n / R, (int32_t)R, (int32_t)(n % R), t, (int32_t)Rw});
    const int32_t nsegs = (int32_t)((p_end - p_begin + kSpecSeg - 1) / kSpecSeg);
    for (int32_t q = 0; q < nsegs; ++q)
      o.fold_items.push_back(SpecFoldItem{p_begin + (int64_t)q * kSpecSeg,
                                          std::min(p_end, p_begin + (int64_t)(q + 1) * kSpecSeg), t, q, nsegs, seg_base});
    seg_base += nsegs;
  }
}

// Decoder block table: the last tensor starting at or before the block, and whether the block
// lies entirely inside it.
void build_dec_blocks(const Desc& d, std::vector<uint32_t>& binfo) {
  const int64_t arena_end = d.offsets[d.nt - 1] + d.sizes[d.nt - 1];
  binfo.assign((size_t)((arena_end + kDecBlk - 1) / kDecBlk), 0u);
  int32_t t = 0;
  for (size_t k = 0; k < binfo.size(); ++k) {
    const int64_t base = (int64_t)k * kDecBlk;
    while (t + 1 < d.nt && d.offsets[t + 1] <= base) ++t;
    const bool inside = d.offsets[t] <= base && base + kDecBlk <= d.offsets[t] + d.sizes[t];
    binfo[k] = (uint32_t)t | (inside ? 0x80000000u : 0u);
  }
}

}  // namespace

bool build_tables(const Desc& d, Tables& o) {
  int64_t np[2];
  build_sequence(d, true, o.enc[0], o.tinfo[0], np[0]);
  build_sequence(d, false, o.enc[1], o.tinfo[1], np[1]);
  build_ring_sequence(d, o);
  build_flat_tables(d, o);
  build_dec_blocks(d, o.dec_binfo);
  o.n_enc[0] = (int64_t)o.enc[0].size();
  o.n_enc[1] = (int64_t)o.enc[1].size();
  o.n_flat = (int64_t)o.flat.size();
  o.n_spec_blocks = 4 * o.n_flat;
  o.n_partials = std::max<int64_t>(std::max(np[0], np[1]), 1);
  return std::max(o.n_enc[0], o.n_spec_blocks) <= 0x7fffffffLL;
}

// Which encoder serves a call, in the order the rules apply:
//   caller norms            the flat quantiser, under every strategy;
//   strategy 4              the grid encoder: on-device draws, any value format and width, arenas of
//                           one launch (larger ones, caller uniforms and the fused PS step take the ring);
//   strategy 3              the bracketed encoder: on-device draws at bit widths 1-4 (fp32 / bf16 /
//                           fp16; the fused PS step and its last client are fp32), and fp32 at 5-8
//                           with wide levels on and no fused last client;
//   the ring                strategies 2 and 4, the fused PS step under any strategy, and strategy 3's
//                           int32-wire fp32 encodes with on-device draws that the bracket does not
//                           serve (Llama-400M s = 8: 0.68 ms against 0.74 for the two-pass encoder);
//   the ticket-ordered one  the rest (bf16 / fp16 and caller uniforms: 0.61 / 0.78 ms against the
//                           ring's 0.70 / 0.83), and every norms-only pass.
Choice choose_encoder(const Call& c) {
  const bool int32_wire = c.bits > 6;  // levels 2^s > 127
  const int32_t ordered = c.strategy >= 2 ? kEncOrdered : c.strategy;
  if (c.norms_only) return {(Encoder)ordered};
  if (c.caller_norms) return {kEncCallerNorms};
  if (c.strategy == 4 && !c.caller_u && !c.divide && c.grid_fits) return {kEncGrid};
  if (c.strategy == 3 && !c.caller_u && c.bits >= kSpecMinBits) {
    const bool wide = c.bits > kSpecMaxBits;
    const bool serves = wide ? !c.last_client && c.wide_levels && c.bits <= kSpecMaxBitsWide && c.fmt == 0
                             : c.fmt == 0 || !c.divide;
    if (serves) {
      const bool skip_bracket = (c.spec_dbg & 1u) != 0;
      const bool fused = c.fused_bracket && !c.last_client && c.fmt == 0 && !skip_bracket;
      return {kEncBracket, wide, fused, !fused && !skip_bracket};
    }
  }
  const bool wide_ring = c.strategy == 3 && int32_wire && !c.caller_u && c.fmt == 0;
  if (c.strategy == 2 || c.strategy == 4 || c.divide || wide_ring) return {kEncRing};
  return {(Encoder)ordered};
}

}  // namespace plan_layout
}  // namespace omf
