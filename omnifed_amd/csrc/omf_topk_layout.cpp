// omf_topk_layout.cpp — the Top-K host tables and carves (omf_topk_layout.h).
#include "omf_topk_layout.h"

#include <algorithm>
#include <cmath>

namespace omf {
namespace topk_layout {

EncodeTables build_encode_tables(const std::vector<int64_t>& sizes, double ratio, int64_t max_runs) {
  const size_t nt = sizes.size();
  EncodeTables tb;
  tb.sizes = sizes;
  tb.kk.resize(nt);
  tb.kb2.resize(nt);
  tb.tfirst.resize(nt);
  tb.tlast.resize(nt);
  tb.koff.assign(nt + 1, 0);
  tb.bbase.assign(nt + 1, 0);
  tb.sbase.assign(nt + 1, 0);
  tb.sblk.assign(nt + 1, 0);
  uint32_t item0 = 0;
  for (size_t t = 0; t < nt; ++t) {
    const int64_t n = sizes[t], k = topk_k(n, ratio);
    const uint32_t ni = (uint32_t)tensor_items(n);
    tb.kk[t] = k;
    tb.koff[t + 1] = tb.koff[t] + k;
    tb.kb2[t] = tb.koff[t] + (int64_t)t * kBucketPad;
    tb.tfirst[t] = item0;
    tb.tlast[t] = item0 + ni - 1;
    tb.bbase[t + 1] = tb.bbase[t] + bucket_slots(k);
    tb.sbase[t + 1] = tb.sbase[t] + tensor_supers(ni);
    const int64_t nr = sample_runs(n, sample_stride(n, max_runs));
    tb.sblk[t + 1] = tb.sblk[t] + sample_blocks(nr);
    for (int64_t r0 = 0; r0 < nr; r0 += kSRunsPerBlock) {
      tb.smap.push_back((uint32_t)t);
      tb.smap.push_back((uint32_t)r0);
    }
    for (uint32_t i = 0; i < ni; i += kSupItems) {
      tb.supinfo.push_back((uint32_t)t);
      tb.supinfo.push_back(item0 + i);
      tb.supinfo.push_back(std::min<uint32_t>(kSupItems, ni - i));
      tb.supinfo.push_back(i == 0 ? 1u : 0u);
    }
    for (int64_t x = 0; x * kZChunk < std::min(k, n); ++x) {  // the zero fill's chunks (zero_fill_chunk)
      tb.zmap.push_back((uint32_t)t);
      tb.zmap.push_back((uint32_t)x);
    }
    item0 += ni;
  }
  tb.nsb = (int32_t)(tb.smap.size() / 2);
  tb.nzb = (int32_t)(tb.zmap.size() / 2);
  return tb;
}

std::vector<Group> make_groups(const EncodeTables& tb, int G) {
  const int32_t nt = (int32_t)tb.sizes.size();
  int64_t total = 0;
  for (int64_t n : tb.sizes) total += n;
  std::vector<Group> gs;
  Group cur;
  int64_t cum = 0;
  for (int32_t t = 0; t < nt; ++t) {
    cur.nb_max = std::max(cur.nb_max, tb.bbase[t + 1] - tb.bbase[t]);
    cum += tb.sizes[t];
    const int g = (int)gs.size();
    if (t == nt - 1 || (g < G - 1 && cum * G >= total * (int64_t)(g + 1))) {  // the group ends with tensor t
      cur.t1 = t + 1;
      cur.nsb = tb.sblk[t + 1] - cur.sb0;
      cur.nsub = (tb.tlast[t] + 1) * (uint32_t)kSubsPerItem - cur.sub0;
      cur.nsup = tb.sbase[t + 1] - cur.sup0;
      cur.nbk = tb.bbase[t + 1] - cur.bk0;
      gs.push_back(cur);
      cur = Group{};
      cur.t0 = t + 1;
      cur.sb0 = tb.sblk[t + 1];
      cur.sub0 = (tb.tlast[t] + 1) * (uint32_t)kSubsPerItem;
      cur.sup0 = tb.sbase[t + 1];
      cur.bk0 = tb.bbase[t + 1];
    }
  }
  return gs;
}

SetupCarve setup_table_carve(const EncodeTables& tb) {
  const size_t nt = tb.sizes.size();
  SetupCarve c;
  OMF_REGION(c.carve, SetupTable, kk, nt);
  OMF_REGION(c.carve, SetupTable, koff, nt + 1);
  OMF_REGION(c.carve, SetupTable, kb2, nt);
  OMF_REGION(c.carve, SetupTable, tfirst, nt);
  OMF_REGION(c.carve, SetupTable, tlast, nt);
  OMF_REGION(c.carve, SetupTable, bbase, nt + 1);
  OMF_REGION(c.carve, SetupTable, sbase, nt + 1);
  OMF_REGION(c.carve, SetupTable, smap, tb.smap.size());
  OMF_REGION(c.carve, SetupTable, supinfo, tb.supinfo.size());
  OMF_REGION(c.carve, SetupTable, zmap, std::max<size_t>(tb.zmap.size(), 2));
  c.zero_begin = c.carve.bytes();
  OMF_REGION(c.carve, SetupTable, done, 4);
  OMF_REGION(c.carve, SetupTable, arrive, nt);
  OMF_REGION(c.carve, SetupTable, gz, nt);
  OMF_REGION(c.carve, SetupTable, gh, nt * kSBins);
  return c;
}

EncodeWsLayout encode_ws_layout(const std::vector<int64_t>& sizes, int64_t arena_end, size_t tmp_bytes) {
  const size_t nt = sizes.size(), ae = (size_t)arena_end;
  size_t n_items = 0, nb_max = 0;
  for (int64_t n : sizes) {
    n_items += (size_t)tensor_items(n);
    nb_max += bucket_slots(n);
  }
  EncodeWsLayout L;
  L.nb_max = nb_max;
  L.tmp_bytes = tmp_bytes;
  auto& c = L.carve;
  // every size below is the one the kernels index (and what the workspace has always held)
  OMF_REGION(c, EncodeWs, hist, nt * kBins);  // exact path: a tensor's histogram; sampled: its redo histogram
  OMF_REGION(c, EncodeWs, bin, nt);           // exact path / exact tail: the tensor's threshold bin
  OMF_REGION(c, EncodeWs, cnt, nt);           // candidates collected per tensor
  OMF_REGION(c, EncodeWs, flag, nt);          // per tensor: redo (sampled path), rewrite (tie order)
  OMF_REGION(c, EncodeWs, status, 16);        // the verdict words [0, 3] and the exact tail's [4, 8]
  L.zero_end = c.bytes();
  OMF_REGION(c, EncodeWs, tkey, nt);          // threshold key
  OMF_REGION(c, EncodeWs, zcnt, nt);          // zeros that complete the selection
  OMF_REGION(c, EncodeWs, seg_b, nt);         // exact path: the tensor's segment of the sort
  OMF_REGION(c, EncodeWs, seg_e, nt);
  OMF_REGION(c, EncodeWs, cstart, nt);        // exact tail: first candidate of the tensor
  OMF_REGION(c, EncodeWs, sub_cnt, n_items * kSubsPerItem);  // candidates per sub-chunk of the fused pass
  OMF_REGION(c, EncodeWs, item_cnt, n_items);
  OMF_REGION(c, EncodeWs, item_off, n_items);
  OMF_REGION(c, EncodeWs, cand, ae);          // a candidate per arena element at most
  // the fallback's packed keys, or the fast path's buckets (k_t + kBucketPad per tensor)
  OMF_REGION(c, EncodeWs, sorted, ae + nt * kBucketPad);
  OMF_REGION(c, EncodeWs, fmap, nt * kCoarse);
  OMF_REGION(c, EncodeWs, tlo, nt);
  OMF_REGION(c, EncodeWs, thi, nt);
  OMF_REGION(c, EncodeWs, fcount, nt);
  OMF_REGION(c, EncodeWs, fhist, nt * kFineMax);
  OMF_REGION(c, EncodeWs, fbucket, nt * kFineMax);
  OMF_REGION(c, EncodeWs, bstart, nb_max);    // the bucket tables: sum of bucket_slots(n_t)
  OMF_REGION(c, EncodeWs, brec, nb_max);
  OMF_REGION(c, EncodeWs, bfill, nb_max);
  OMF_REGION(c, EncodeWs, tmp, tmp_bytes);
  L.total = c.bytes();
  return L;
}

DecodeTables dec_tables_host(const std::vector<int64_t>& sizes, const std::vector<int64_t>& offsets,
                             int64_t arena_end, const int64_t* ks) {
  const int32_t nt = (int32_t)sizes.size();
  DecodeTables d;
  d.nsuper = dec_nsuper(arena_end);
  d.koff.assign((size_t)nt + 1, 0);
  std::vector<double> expect((size_t)d.nsuper, 0.0);
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t n = sizes[t], k = ks[t];
    d.koff[(size_t)t + 1] = d.koff[(size_t)t] + k;
    if (n <= 0 || k <= 0) continue;
    const int64_t begin = offsets[t];
    const double dens = (double)k / (double)n;
    for (int64_t s0 = begin >> kDecSuperBits; s0 <= (begin + n - 1) >> kDecSuperBits; ++s0) {
      const int64_t lo = std::max(begin, s0 << kDecSuperBits), hi = std::min(begin + n, (s0 + 1) << kDecSuperBits);
      expect[(size_t)s0] += dens * (double)(hi - lo);
    }
  }
  d.cap_base.assign((size_t)d.nsuper + 1, 0);
  for (int32_t q = 0; q < d.nsuper; ++q) {
    const uint64_t cap = std::min<uint64_t>((uint64_t)std::ceil(2.0 * expect[(size_t)q]) + 256, (uint64_t)1 << kDecSuperBits);
    d.cap_base[(size_t)q + 1] = d.cap_base[(size_t)q] + (uint32_t)cap;
  }
  const int64_t ktot = d.koff[(size_t)nt];
  const int64_t nb = dec_place_blocks(ktot);
  d.blk_t.assign(2 * (size_t)nb, 0);
  auto tensor_of = [&](int64_t j) {  // the largest t with koff[t] <= j, as koff_tensor on the device
    return (uint32_t)(std::upper_bound(d.koff.begin(), d.koff.begin() + nt, j) - d.koff.begin() - 1);
  };
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t j0 = b * kDecChunk, j1 = std::max<int64_t>(std::min<int64_t>(j0 + kDecChunk, ktot), j0 + 1);
    d.blk_t[2 * (size_t)b] = tensor_of(j0);
    d.blk_t[2 * (size_t)b + 1] = tensor_of(j1 - 1);
  }
  return d;
}

Carve<DecTable> dec_table_carve(int32_t nt, int32_t nsuper, int64_t place_blocks) {
  Carve<DecTable> c;
  OMF_REGION(c, DecTable, koff, (size_t)nt + 1);
  OMF_REGION(c, DecTable, cap_base, (size_t)nsuper + 1);
  OMF_REGION(c, DecTable, blk_t, 2 * (size_t)place_blocks);
  return c;
}

Carve<DecWs> dec_ws_layout(int32_t nsuper, uint64_t cap_total, int64_t ktot) {
  Carve<DecWs> c;
  OMF_REGION(c, DecWs, fill, (size_t)nsuper + 1);  // + the overflow count
  OMF_REGION(c, DecWs, pairs, (size_t)std::max<uint64_t>(cap_total, 1));
  OMF_REGION(c, DecWs, ovf, (size_t)std::max<int64_t>(ktot, 1));
  return c;
}

PackTables pack_tables_host(const std::vector<int64_t>& sizes, const int64_t* ks) {
  const size_t nt = sizes.size();
  PackTables p;
  p.bits.resize(nt);
  p.koff.assign(nt + 1, 0);
  p.goff.assign(nt + 1, 0);
  p.woff.assign(nt + 1, 0);
  bool ok = true;
  for (size_t t = 0; t < nt; ++t) {
    const int32_t b = index_bits(sizes[t]);
    const int64_t groups = (ks[t] + kPackGroup - 1) / kPackGroup;
    p.bits[t] = b;
    p.koff[t + 1] = p.koff[t] + ks[t];
    p.goff[t + 1] = p.goff[t] + groups;
    p.woff[t + 1] = p.woff[t] + (b > 0 ? groups * b : 0);
    ok = ok && b > 0;
  }
  p.words = ok ? p.woff[nt] : -1;
  return p;
}

Carve<PackTable> pack_table_carve(int32_t nt) {
  Carve<PackTable> c;
  OMF_REGION(c, PackTable, koff, (size_t)nt + 1);
  OMF_REGION(c, PackTable, woff, (size_t)nt + 1);
  OMF_REGION(c, PackTable, goff, (size_t)nt + 1);
  OMF_REGION(c, PackTable, bits, (size_t)nt);
  return c;
}

}  // namespace topk_layout
}  // namespace omf
