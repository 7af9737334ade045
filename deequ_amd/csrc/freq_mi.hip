// freq_mi.hip -- marginals of a two-key frequency table and MutualInformation over it
// (freq_table.h has the group-by's overview): dq_freq_marginal, dq_freq_mutual_information and
// their kernels.
#include "freq_table.h"

// The kernels and their argument structs below (SmallEntry, Lookup, CountSlot, CountIndex) are at
// global scope, not in namespace dq, as they always were: their symbol names stay as they are.
using namespace dq;

// str_row_hash of an arena-encoded utf8 part (tag, length, bytes zero-padded to 4): the bytes
// start dword-aligned, so a key of <= 16 bytes is read as its dwords (no byte loop), masked to its
// length, and hashed from registers (str_row_hash_reg == str_row_hash for such keys).
DQ_DEV uint64_t enc_str_hash(const uint32_t* part) {
  const int32_t len = (int32_t)part[1];
  if (len > 16) return str_row_hash(SView{reinterpret_cast<const uint8_t*>(part + 2), len});
  const int nd = (len + 3) >> 2;
  uint32_t d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = k < nd ? part[2 + k] : 0u;
  const uint32_t tail = (uint32_t)len & 3u;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tail && k == nd - 1) d[k] &= (1u << (8 * tail)) - 1u;
  const uint64_t w0 = (uint64_t)d[0] | ((uint64_t)d[1] << 32);
  const uint64_t w1 = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
  return str_row_hash_reg(w0, w1, len);
}

// The marginal of key column k over a hashed table's groups, as records for a one-key table:
// column k's part of a group's encoded key IS the one-column encoding of that value, so a
// record points into the same arena (enc_off), and carries the group's count.  Exact output
// (fixed-width column): key = the value.  Hashed output (utf8): key = the one-column row hash.
__global__ void freq_project(const Group* __restrict__ g, int64_t n, const uint8_t* __restrict__ arena,
                             PartTypes t, int k, RecIn* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* enc = reinterpret_cast<const uint32_t*>(arena + g[i].rep);
  uint32_t w = 0;
  for (int c = 0; c < k; ++c) {  // skip the columns before k
    const uint32_t tag = enc[w++];
    if (!tag) continue;
    if (t.types[c] == DQ_UTF8) w += 1 + pad4(enc[w]) / 4;
    else w += 2;
  }
  RecIn r;
  r.count = g[i].count;
  r.enc_off = g[i].rep + 4ull * w;
  if (t.types[k] == DQ_UTF8) {
    r.key = enc_str_hash(enc + w);
  } else {
    r.key = (uint64_t)enc[w + 1] | ((uint64_t)enc[w + 2] << 32);
  }
  out[i] = r;
}

// Both marginals' records of a two-key table's groups in one pass over the groups and the arena
// (freq_project for key 0 and key 1).
__global__ void freq_project2(const Group* __restrict__ g, int64_t n, const uint8_t* __restrict__ arena,
                              PartTypes t, RecIn* __restrict__ out0, RecIn* __restrict__ out1) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Group gi = g[i];
  const uint32_t* enc = reinterpret_cast<const uint32_t*>(arena + gi.rep);
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    RecIn r;
    r.count = gi.count;
    r.enc_off = gi.rep + 4ull * w;
    const uint32_t tag = enc[w];
    if (t.types[k] == DQ_UTF8) {
      r.key = enc_str_hash(enc + w);
      w += tag ? 2 + pad4(enc[w + 1]) / 4 : 1;
    } else {
      r.key = (uint64_t)enc[w + 1] | ((uint64_t)enc[w + 2] << 32);
      w += tag ? 3 : 1;
    }
    RecIn* o = k ? out1 : out0;  // (nullptr: that side's marginal is built another way)
    if (o) o[i] = r;
  }
}

// ---- small marginals (MutualInformation over a low-cardinality column) ----------------------------
// One pass over the joint groups aggregates each side's marginal in registers and LDS when the
// side has at most kSmallMarg distinct values per wave and keys of at most 8 encoded words: a wave
// keeps its values (row hash + encoded words), matches every group's part against them (hash and
// words), and sums the joint counts per value with one wave reduction per value.  The host merges
// the waves' lists by (hash, words).  A side with more values, a longer key or two values on one
// hash is marked failed and takes the general path (a one-key table of the projected records).
// Also writes every group's row hash of each side (hk[k][i], the hash its marginal is indexed by).
constexpr int kSmallMarg = 16;
struct SmallEntry {
  unsigned long long h, count;
  uint32_t w[8];
};
// freq_small_marginal's per-wave lists of the small sides merged on the device (one workgroup per
// side): values claimed by hash in an LDS table, counts added, then every entry's words checked
// against the first entry of its hash -- the host reads a few KB instead of every wave's list (12.6
// MB for a 1.2e8-group joint, ~4 ms of copies and map inserts).  out_n[k]: the merged values, or
// kSmallMergeHost (more values than the table takes: the host merges the lists as before), or
// kSmallMergeClash (two values on one hash, or the side failed: not small).
constexpr int kSmallMergeSlots = 1024, kSmallMerged = 512;
constexpr uint32_t kSmallMergeHost = 0xFFFFFFFFu, kSmallMergeClash = 0xFFFFFFFEu;
__global__ void __launch_bounds__(1024) freq_small_merge(const SmallEntry* __restrict__ ent,
                                                         const uint32_t* __restrict__ nout, int64_t nw,
                                                         const unsigned int* __restrict__ fail,
                                                         SmallEntry* __restrict__ out, uint32_t* __restrict__ out_n) {
  constexpr int S = kSmallMergeSlots;
  constexpr unsigned long long kFree = ~0ULL;
  __shared__ unsigned long long s_h[S], s_c[S], s_first[S];
  __shared__ uint32_t s_w[S][8];
  __shared__ uint32_t s_full, s_clash;
  const int k = blockIdx.x, tid = threadIdx.x;
  if (fail[k]) {
    if (tid == 0) out_n[k] = kSmallMergeClash;
    return;
  }
  for (int i = tid; i < S; i += blockDim.x) {
    s_h[i] = kFree;
    s_c[i] = 0;
    s_first[i] = kFree;
  }
  if (tid == 0) s_full = s_clash = 0;
  __syncthreads();
  // the slot of entry x's hash (claimed when `claim`), or S: none / the table is full
  auto slot_of = [&](const SmallEntry& e, bool claim) -> uint32_t {
    uint32_t sl = (uint32_t)e.h & (S - 1);
    for (int pr = 0; pr < S; ++pr, sl = (sl + 1) & (S - 1)) {
      const unsigned long long old = claim ? atomicCAS(&s_h[sl], kFree, e.h) : s_h[sl];
      if (old == e.h || (claim && old == kFree)) return sl;
      if (!claim && old == kFree) return S;
    }
    return S;
  };
  // a thread per wave list (its count read once); f(e, x) for each entry x of side k
  auto for_entries = [&](auto&& f) {
    for (int64_t gwv = tid; gwv < nw; gwv += blockDim.x) {
      const uint32_t nl = nout[gwv * 2 + k];
      for (uint32_t c = 0; c < nl; ++c) f(ent[(gwv * 2 + k) * kSmallMarg + c], gwv * kSmallMarg + c);
    }
  };
  for_entries([&](const SmallEntry& e, int64_t x) {  // claims, counts, the first entry per value
    const uint32_t sl = e.h == kFree ? (uint32_t)S : slot_of(e, true);
    if (sl == (uint32_t)S) {
      s_full = 1;
      return;
    }
    atomicAdd(&s_c[sl], e.count);
    atomicMin(&s_first[sl], (unsigned long long)x);
  });
  __syncthreads();
  if (s_full) {
    if (tid == 0) out_n[k] = kSmallMergeHost;
    return;
  }
  for_entries([&](const SmallEntry& e, int64_t x) {  // the first entry of each value: its words
    const uint32_t sl = slot_of(e, false);
    if (sl < (uint32_t)S && s_first[sl] == (unsigned long long)x)
      for (int q = 0; q < 8; ++q) s_w[sl][q] = e.w[q];
  });
  __syncthreads();
  for_entries([&](const SmallEntry& e, int64_t) {  // every entry's words against its value's
    const uint32_t sl = slot_of(e, false);
    bool eq = sl < (uint32_t)S;
    for (int q = 0; q < 8 && eq; ++q) eq = s_w[sl][q] == e.w[q];
    if (!eq) s_clash = 1;
  });
  __syncthreads();
  if (tid == 0) {
    uint32_t m = 0;
    for (int sl = 0; sl < S && m <= (uint32_t)kSmallMerged; ++sl) {
      if (s_h[sl] == kFree) continue;
      if (m < (uint32_t)kSmallMerged) {
        SmallEntry o;
        o.h = s_h[sl];
        o.count = s_c[sl];
        for (int j = 0; j < 8; ++j) o.w[j] = s_w[sl][j];
        out[(int64_t)k * kSmallMerged + m] = o;
      }
      ++m;
    }
    out_n[k] = s_clash ? kSmallMergeClash : (m > (uint32_t)kSmallMerged ? kSmallMergeHost : m);
  }
}

// A side's part of an encoded key from the 16 words loaded at the key's start: its word count,
// its row hash (utf8 <= 16 bytes and fixed-width from the words; longer utf8 from memory) and
// its first 8 words (a side with a longer key is not aggregated here)
DQ_DEV void small_part(const uint32_t (&e)[16], uint32_t w, bool utf8, const uint32_t* enc, uint32_t& nw,
                       uint64_t& h, uint32_t (&pw)[8]) {
  uint32_t ww[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) {  // e[w + j] (w <= 6 for a first side of <= 8 words... else memory)
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) v = (uint32_t)q == w + (uint32_t)j ? e[q] : v;
    ww[j] = w + (uint32_t)j < 16u ? v : enc[w + j];
  }
  const uint32_t tag = ww[0];
  if (utf8) {
    const uint32_t len = ww[1];
    nw = tag ? 2u + pad4(len) / 4 : 1u;
    if (!tag) {
      h = 0;
    } else if (len <= 16) {
      const int nd = (int)((len + 3) >> 2);
      uint32_t d[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = k < nd ? ww[2 + k] : 0u;
      const uint32_t tail = len & 3u;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (tail && k == nd - 1) d[k] &= (1u << (8 * tail)) - 1u;
      h = str_row_hash_reg((uint64_t)d[0] | ((uint64_t)d[1] << 32), (uint64_t)d[2] | ((uint64_t)d[3] << 32),
                           (int32_t)len);
    } else {
      h = enc_str_hash(enc + w);
    }
  } else {
    nw = tag ? 3u : 1u;
    h = tag ? fmix_bij((uint64_t)ww[1] | ((uint64_t)ww[2] << 32)) : 0;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) pw[j] = (uint32_t)j < nw ? ww[j] : 0u;
}

__global__ void __launch_bounds__(256)
freq_small_marginal(const Group* __restrict__ g, int64_t n, const uint8_t* __restrict__ arena, PartTypes t,
                    uint32_t try_sides, unsigned long long* __restrict__ hk0, unsigned long long* __restrict__ hk1,
                    SmallEntry* __restrict__ out, uint32_t* __restrict__ nout, unsigned int* __restrict__ fail,
                    RecIn* __restrict__ rec0, RecIn* __restrict__ rec1) {
  __shared__ unsigned long long s_h[4][2][kSmallMarg], s_c[4][2][kSmallMarg];
  __shared__ uint32_t s_w[4][2][kSmallMarg][8];
  constexpr int U = 2;  // groups per lane per step, every load of the step in flight together
  const int lane = (int)__lane_id(), wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave;
  int nc[2] = {0, 0};
  bool dead[2] = {!(try_sides & 1u), !(try_sides & 2u)};
  for (int64_t base = gw * 64 * U; base < n; base += (int64_t)gridDim.x * 256 * U) {
    Group gi[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * 64 + lane;
      on[u] = i < n;
      gi[u] = g[on[u] ? i : n - 1];
    }
    uint32_t e[U][16];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t* enc = reinterpret_cast<const uint32_t*>(arena + gi[u].rep);
#pragma unroll
      for (int q = 0; q < 16; ++q) e[u][q] = enc[q];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * 64 + lane;
      const uint32_t* enc = reinterpret_cast<const uint32_t*>(arena + gi[u].rep);
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        uint32_t nw, pw[8];
        uint64_t h;
        small_part(e[u], w, t.types[k] == DQ_UTF8, enc, nw, h, pw);
        if (on[u]) (k ? hk1 : hk0)[i] = h;
        RecIn* ro = k ? rec1 : rec0;  // freq_project2's record of this side, for a general marginal
        if (ro && on[u]) {            // (a utf8 part's key hash is its row hash)
          RecIn r;
          r.key = t.types[k] == DQ_UTF8 ? h : ((uint64_t)pw[1] | ((uint64_t)pw[2] << 32));
          r.count = gi[u].count;
          r.enc_off = gi[u].rep + 4ull * w;
          ro[i] = r;
        }
        if (!dead[k] && __ballot(on[u] && (!pw[0] || nw > 8u))) dead[k] = true;  // NULL part, long key
        if (!dead[k]) {
          int m = -1;
          for (int c = 0; c < nc[k]; ++c) {
            bool eq = on[u] && m < 0 && s_h[wave][k][c] == h;
#pragma unroll
            for (int j = 0; j < 8; ++j) eq = eq && s_w[wave][k][c][j] == pw[j];
            if (eq) m = c;
          }
          while (true) {
            const uint64_t need = __ballot(on[u] && m < 0);
            if (!need) break;
            if (nc[k] == kSmallMarg) {
              dead[k] = true;
              break;
            }
            const int leader = __builtin_ctzll(need);
            const uint64_t lh = ((uint64_t)__builtin_amdgcn_readlane((int)(h >> 32), leader) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h, leader);
            uint32_t lw[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) lw[j] = (uint32_t)__builtin_amdgcn_readlane((int)pw[j], leader);
            bool clash = false;  // another value on this hash: not decidable by hash
            for (int c = 0; c < nc[k]; ++c) clash = clash || s_h[wave][k][c] == lh;
            if (clash) {
              dead[k] = true;
              break;
            }
            const int c = nc[k]++;
            if (lane == 0) {
              s_h[wave][k][c] = lh;
              s_c[wave][k][c] = 0;
#pragma unroll
              for (int j = 0; j < 8; ++j) s_w[wave][k][c][j] = lw[j];
            }
            bool eq = on[u] && m < 0 && h == lh;
#pragma unroll
            for (int j = 0; j < 8; ++j) eq = eq && pw[j] == lw[j];
            if (eq) m = c;
          }
          if (!dead[k]) {
            for (int c = 0; c < nc[k]; ++c) {
              const uint64_t sum = __ockl_wfred_add_u64(m == c ? gi[u].count : 0ULL);
              if (lane == 0) s_c[wave][k][c] += sum;
            }
          }
        }
        w += nw;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int64_t slot = gw * 2 + k;
    if (dead[k]) {
      if (lane == 0) {
        nout[slot] = 0u;
        if (try_sides & (1u << k)) atomicOr(&fail[k], 1u);
      }
      continue;
    }
    if (lane < nc[k]) {
      SmallEntry en;
      en.h = s_h[wave][k][lane];
      en.count = s_c[wave][k][lane];
#pragma unroll
      for (int j = 0; j < 8; ++j) en.w[j] = s_w[wave][k][lane][j];
      out[slot * kSmallMarg + lane] = en;
    }
    if (lane == 0) nout[slot] = (uint32_t)nc[k];
  }
}

// ---- MutualInformation (MutualInformation.scala:41-84) -----------------------------------------
// Column k's part of an encoded multi-key group key.
DQ_DEV const uint32_t* enc_part(const uint32_t* enc, const PartTypes& t, int k) {
  uint32_t w = 0;
  for (int c = 0; c < k; ++c) {
    const uint32_t tag = enc[w++];
    if (!tag) continue;
    if (t.types[c] == DQ_UTF8) w += 1 + pad4(enc[w]) / 4;
    else w += 2;
  }
  return enc + w;
}

// Open-addressing index over a one-key table's groups: slot -> group index + 1 (0 = empty).
struct Lookup {
  const Group* g;
  const uint32_t* slots;
  uint64_t mask;
  const uint8_t* arena;
  int32_t type;
  int32_t exact;
  // a marginal group's rep = rep_base + the joint-arena offset of the key part it was made
  // from (dq_freq_marginal copies the joint arena): a part at that offset IS the group's key
  uint64_t rep_base;
};

__global__ void freq_lookup_build(const Group* __restrict__ g, int64_t n, uint64_t mask,
                                  uint32_t* __restrict__ slots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t s = g[i].h & mask;
  while (atomicCAS(&slots[s], 0u, (uint32_t)(i + 1)) != 0u) s = (s + 1) & mask;
}

// The count of the marginal group whose key is the one-column encoding `part`, at offset
// part_off of the joint arena.
DQ_DEV uint64_t lookup_count(const Lookup& L, const uint32_t* part, uint64_t part_off) {
  uint64_t h;
  if (L.exact) {
    h = fmix_bij((uint64_t)part[1] | ((uint64_t)part[2] << 32));
  } else {
    h = enc_str_hash(part);
  }
  for (uint64_t s = h & L.mask;; s = (s + 1) & L.mask) {
    const uint32_t idx = L.slots[s];
    if (!idx) return 0;  // not reachable: every joint value has its marginal group
    const Group& m = L.g[idx - 1];
    if (m.h != h) continue;
    if (L.exact || m.rep == L.rep_base + part_off) return m.count;  // (its own record: no compare)
    const int32_t ty = DQ_UTF8;
    if (enc_equal_arena(reinterpret_cast<const uint32_t*>(L.arena + m.rep), part, &ty, 1)) return m.count;
  }
}

// terms[i] = (pxy/n) ln((pxy/n) / ((px/n)(py/n))), the reference's UDF (MutualInformation.scala:
// 61-64) with its operation order, per joint group
__global__ void freq_mi_terms(const Group* __restrict__ gj, int64_t n, const uint8_t* __restrict__ arena,
                              PartTypes t, Lookup X, Lookup Y, double total, double* __restrict__ terms) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* enc = reinterpret_cast<const uint32_t*>(arena + gj[i].rep);
  const uint32_t* ex = enc_part(enc, t, 0);
  const uint32_t* ey = enc_part(enc, t, 1);
  const double px = (double)lookup_count(X, ex, gj[i].rep + 4ull * (uint64_t)(ex - enc));
  const double py = (double)lookup_count(Y, ey, gj[i].rep + 4ull * (uint64_t)(ey - enc));
  const double pxy = (double)gj[i].count;
  terms[i] = (pxy / total) * log((pxy / total) / ((px / total) * (py / total)));
}

// A marginal's groups by row hash, for a table with no two keys on one 64-bit hash (its phase C
// counted no collision): slot = {row hash, count}, count 0 = empty, so a lookup is one probe
// sequence with no key bytes compared.
struct CountSlot {
  unsigned long long h, count;
};
// -sum (c/n) ln(c/n) over a small marginal's value counts (count 0: an empty slot), as the
// fixed-point sum phase C keeps (entropy_term compiled from the same text, freq_device.h, so the same bits as a table's)
__global__ void __launch_bounds__(256) freq_slots_entropy(const CountSlot* __restrict__ t, uint64_t n_slots,
                                                          double num_rows, unsigned long long* out) {
  fix128 e = 0;
  for (uint64_t i = threadIdx.x; i < n_slots; i += 256)
    if (t[i].count) e += fix_of(entropy_term(t[i].count, num_rows));
  e = wave_sum_fix(e);
  if (__lane_id() == 0 && e) atomic_add_fix(out, e);
}
__global__ void freq_count_index(const Group* __restrict__ g, int64_t n, uint64_t mask,
                                 CountSlot* __restrict__ slots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Group gi = g[i];
  uint64_t s = gi.h & mask;
  while (atomicCAS(&slots[s].count, 0ULL, (unsigned long long)gi.count) != 0ULL) s = (s + 1) & mask;
  slots[s].h = gi.h;
}
// Per-partition form (the marginal's phase C partitions, built in LDS, no global atomics):
// partition p = h >> part_shift owns slots [pbase[p], pbase[p] + 2^plog[p]), probed from h's low
// bits.  pbase == nullptr: one table of mask + 1 slots.
struct CountIndex {
  const CountSlot* slots;
  uint64_t mask;
  const unsigned long long* pbase;
  const uint8_t* plog;
  int part_shift;
};
constexpr int kIdxMaxLog = 12;  // the largest per-partition table built in LDS (64 KB)
__global__ void __launch_bounds__(256)
freq_count_index_parts(const Group* __restrict__ groups, const unsigned long long* __restrict__ part_off,
                       const unsigned long long* __restrict__ part_groups, int64_t P,
                       const unsigned long long* __restrict__ pbase, const uint8_t* __restrict__ plog,
                       CountSlot* __restrict__ slots) {
  __shared__ unsigned long long s_h[1 << kIdxMaxLog], s_c[1 << kIdxMaxLog];
  for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
    const uint32_t R = 1u << plog[p];
    const uint64_t off = part_off[p], n = part_groups[p];
    for (uint32_t j = threadIdx.x; j < R; j += 256) s_c[j] = 0;
    __syncthreads();
    for (uint64_t i = threadIdx.x; i < n; i += 256) {
      const Group gi = groups[off + i];
      uint32_t sl = (uint32_t)gi.h & (R - 1);
      while (atomicCAS(&s_c[sl], 0ULL, (unsigned long long)gi.count) != 0ULL) sl = (sl + 1) & (R - 1);
      s_h[sl] = gi.h;
    }
    __syncthreads();
    CountSlot* out = slots + pbase[p];
    for (uint32_t j = threadIdx.x; j < R; j += 256) out[j] = CountSlot{s_c[j] ? s_h[j] : 0ULL, s_c[j]};
    __syncthreads();
  }
}
DQ_DEV uint64_t count_of(const CountIndex& x, uint64_t h) {
  const CountSlot* sl = x.slots;
  uint64_t mask = x.mask;
  if (x.pbase) {
    const uint64_t p = h >> x.part_shift;
    sl += x.pbase[p];
    mask = (1ULL << x.plog[p]) - 1;
  }
  for (uint64_t s = h & mask;; s = (s + 1) & mask) {
    const CountSlot c = sl[s];
    if (c.h == h || c.count == 0) return c.count;  // (count 0: not reachable, every joint value has its group)
  }
}
// freq_mi_terms with both marginals looked up by the row hashes the projection computed (exact
// keys: the bijective hash of the value), same arithmetic and order
// (k0 / k1: each side's key of group i at k[i * stride]: a RecIn's key (stride 3; exact: the
// value, hashed here) or freq_small_marginal's row hash (stride 1))
__global__ void freq_mi_terms_h(const Group* __restrict__ gj, int64_t n, const uint64_t* __restrict__ k0,
                                int st0, const uint64_t* __restrict__ k1, int st1, int exact0, int exact1,
                                CountIndex x0, CountIndex x1, double total, double* __restrict__ terms) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h0 = exact0 ? fmix_bij(k0[i * st0]) : k0[i * st0];
  const uint64_t h1 = exact1 ? fmix_bij(k1[i * st1]) : k1[i * st1];
  const double px = (double)count_of(x0, h0);
  const double py = (double)count_of(x1, h1);
  const double pxy = (double)gj[i].count;
  terms[i] = (pxy / total) * log((pxy / total) / ((px / total) * (py / total)));
}

// Order-independent sum of the MutualInformation terms (the joint groups' order is phase C's
// output order, which varies from run to run): each term in fixed point (fix_of), summed as
// integers; a non-finite term (a marginal count that is not there) is added as a double beside
// (NaN / inf sums do not depend on order either).  partial[b] = {lo, hi, non-finite sum bits}.
__global__ void __launch_bounds__(256) freq_sum_fix(const double* __restrict__ x, int64_t n,
                                                    unsigned long long* __restrict__ partial) {
  __shared__ fix128 s_red[256 / 64];
  __shared__ double s_nf[256 / 64];
  fix128 acc = 0;
  double nf = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double t = x[i];
    if (fabs(t) < 16384.0) acc += fix_of(t);
    else nf += t;  // (NaN fails the test too)
  }
  acc = wave_sum_fix(acc);
  nf = block_sum_f64(nf, s_nf);
  if (__lane_id() == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    fix128 t = 0;
    for (int w = 0; w < 256 / 64; ++w) t += s_red[w];
    store_fix(partial + 3 * blockIdx.x, t);
    partial[3 * blockIdx.x + 2] = __builtin_bit_cast(unsigned long long, nf);
  }
}

// borrow: the marginal reads the joint table's arena in place (it must die first)
static dq_status marginal_of(dq_freq* joint, int key_index, dq_freq* out, void* hip_stream,
                             bool borrow) {
  if (!joint || !out) return fail(DQ_ERR_INVALID_ARGUMENT, "null argument");
  if (joint->exact || joint->n_keys < 2) return fail(DQ_ERR_INVALID_ARGUMENT, "not a multi-key table");
  if (key_index < 0 || key_index >= joint->n_keys) return fail(DQ_ERR_INVALID_ARGUMENT, "bad key index");
  if (out->n_keys != 1 || out->logical[0] != joint->logical[key_index])
    return fail(DQ_ERR_WRONG_TYPE, "the marginal table must have one key of the column's type");
  if (joint->mode_null_as_group > 0) return fail(DQ_ERR_UNSUPPORTED, "marginal of a Histogram table");
  HIP_TRY(hipSetDevice(joint->device));
  dq_status st = compact_groups(joint);
  if (st != DQ_OK) return st;
  const int64_t n = joint->n_compact;
  DevBuf<RecIn> rec;
  HIP_TRY(rec.ensure(std::max<int64_t>(n, 1)));
  if (n) {
    hipLaunchKernelGGL(freq_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, joint->stream,
                       joint->compact.p, n, arena_of(joint), part_types(joint, 1), key_index, rec.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(joint->stream));
  }
  const int dbg = freq_debug_level();
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t rc[1] = {n};
  const int64_t vb[1] = {(int64_t)((joint->arena_used + 7) & ~7ULL)};
  const int64_t special[3] = {0, 0, (int64_t)joint->h_counters[C_NULL_ROWS]};
  st = add_records(out, reinterpret_cast<const dq_freq_record*>(rec.p), arena_of(joint), 1, rc, vb,
                   joint->num_rows, special, 0, hip_stream, borrow && !out->exact);
  if (st != DQ_OK) return st;
  HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(hip_stream)));
  if (dbg)
    fprintf(stderr, "dq_freq marginal %d: records added in %.2f ms\n", key_index,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return DQ_OK;
}

extern "C" dq_status dq_freq_marginal(dq_freq* joint, int key_index, dq_freq* out,
                                     void* hip_stream) {
  return marginal_of(joint, key_index, out, hip_stream, false);
}

extern "C" dq_status dq_freq_mutual_information(dq_freq* joint, double* mi, int* is_null,
                                               void* hip_stream) {
  if (!joint || !mi || !is_null) return fail(DQ_ERR_INVALID_ARGUMENT, "null argument");
  if (joint->exact || joint->n_keys != 2)
    return fail(DQ_ERR_INVALID_ARGUMENT, "MutualInformation needs a two-key grouping table");
  HIP_TRY(hipSetDevice(joint->device));
  dq_status st = compact_groups(joint);
  if (st != DQ_OK) return st;
  const int64_t n = joint->n_compact;
  *mi = 0.0;
  *is_null = n == 0 ? 1 : 0;  // sum over no joint groups is NULL
  if (!n) return DQ_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
  const int dbg = freq_debug_level();  // the MI pass's steps, timed (synchronising)
  auto t_last = std::chrono::steady_clock::now();
  auto stamp = [&](const char* what) {
    if (!dbg) return;
    (void)hipStreamSynchronize(stream);
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "dq_freq MI %s: %.2f ms\n", what,
            std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  dq_freq* marg[2] = {nullptr, nullptr};
  DevBuf<uint32_t> slots[2];
  DevBuf<CountSlot> cslots[2];
  uint64_t cmask[2] = {0, 0};
  Lookup L[2];
  dq_status res = DQ_OK;
  const char* fl = getenv("DQ_FREQ_MI_LOOKUP");  // =1: the byte-compare lookups (A/B, tests)
  const bool force_lookup = fl && atoi(fl) != 0;
  const char* fsm = getenv("DQ_FREQ_MI_NOSMALL");  // =1: no small-marginal pass (A/B, tests)
  bool small[2] = {false, false};  // side k's marginal aggregated by freq_small_marginal
  DevBuf<unsigned long long> hk[2];
  // each side's records of the joint groups (kept: the lookups read their keys), written by the
  // small-marginal pass for both sides (a side that is not small needs them; otherwise
  // freq_project2 makes them in a pass of its own)
  DevBuf<RecIn> rec[2];
  bool rec_done = false;
  if (!force_lookup && !(fsm && atoi(fsm))) {
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((n + 511) / 512, 1), 2048);
    const int64_t nw = (int64_t)grid * 4;
    DevBuf<SmallEntry> ent;
    DevBuf<uint32_t> nout;
    DevBuf<unsigned int> sfail;
    HIP_TRY(hk[0].ensure(n));
    HIP_TRY(hk[1].ensure(n));
    HIP_TRY(ent.ensure((size_t)nw * 2 * kSmallMarg));
    HIP_TRY(nout.ensure((size_t)nw * 2));
    HIP_TRY(sfail.ensure(2));
    HIP_TRY(rec[0].ensure(n));
    HIP_TRY(rec[1].ensure(n));
    HIP_TRY(hipMemsetAsync(sfail.p, 0, 8, stream));
    hipLaunchKernelGGL(freq_small_marginal, dim3(grid), dim3(256), 0, stream, joint->compact.p, n,
                       arena_of(joint), part_types(joint, 1), 3u, hk[0].p, hk[1].p, ent.p, nout.p, sfail.p,
                       rec[0].p, rec[1].p);
    HIP_TRY(hipGetLastError());
    rec_done = true;
    unsigned int hf[2];
    HIP_TRY(d2h(hf, sfail.p, 8, stream));
    if (!hf[0] || !hf[1]) {  // merge the waves' lists of each small side by (hash, words)
      DevBuf<SmallEntry> mo;
      DevBuf<uint32_t> mn;
      HIP_TRY(mo.ensure(2 * (size_t)kSmallMerged));
      HIP_TRY(mn.ensure(2));
      hipLaunchKernelGGL(freq_small_merge, dim3(2), dim3(1024), 0, stream, ent.p, nout.p, nw, sfail.p, mo.p, mn.p);
      HIP_TRY(hipGetLastError());
      uint32_t hm[2];
      HIP_TRY(d2h(hm, mn.p, 8, stream));
      const char* hmg = getenv("DQ_FREQ_MI_HOSTMERGE");  // =1: the host merge (A/B, tests)
      if (hmg && atoi(hmg))
        for (int k = 0; k < 2; ++k)
          if (hm[k] != kSmallMergeClash) hm[k] = kSmallMergeHost;
      std::vector<SmallEntry> hme(2 * (size_t)kSmallMerged);
      HIP_TRY(d2h(hme.data(), mo.p, hme.size() * sizeof(SmallEntry), stream));
      // (the host merge of every wave's list, for a side the device table could not take)
      std::vector<uint32_t> hn;
      std::vector<SmallEntry> he;
      if ((!hf[0] && hm[0] == kSmallMergeHost) || (!hf[1] && hm[1] == kSmallMergeHost)) {
        hn.resize((size_t)nw * 2);
        he.resize((size_t)nw * 2 * kSmallMarg);
        HIP_TRY(d2h(hn.data(), nout.p, hn.size() * 4, stream));
        HIP_TRY(d2h(he.data(), ent.p, he.size() * sizeof(SmallEntry), stream));
      }
      for (int k = 0; k < 2; ++k) {
        if (hf[k] || hm[k] == kSmallMergeClash) continue;
        const bool host = hm[k] == kSmallMergeHost;
        // (merged on the device: one list of hm[k] entries, as if from one wave)
        const int64_t lists = host ? nw : 1;
        std::map<uint64_t, std::pair<std::array<uint32_t, 8>, uint64_t>> vals;
        bool ok = true;
        for (int64_t gwv = 0; gwv < lists && ok; ++gwv)
          for (uint32_t c = 0; c < (host ? hn[gwv * 2 + k] : hm[k]) && ok; ++c) {
            const SmallEntry& e = host ? he[((size_t)gwv * 2 + k) * kSmallMarg + c]
                                       : hme[(size_t)k * kSmallMerged + c];
            std::array<uint32_t, 8> wv;
            for (int q = 0; q < 8; ++q) wv[q] = e.w[q];
            auto it = vals.find(e.h);
            if (it == vals.end()) vals.emplace(e.h, std::make_pair(wv, (uint64_t)e.count));
            else if (it->second.first != wv) ok = false;  // two values on one hash
            else it->second.second += e.count;
          }
        if (!ok) continue;
        uint64_t cap = 2;
        while (cap < 2 * (uint64_t)vals.size()) cap <<= 1;
        std::vector<CountSlot> tab(cap, CountSlot{0, 0});
        for (const auto& kv : vals) {
          uint64_t sl = kv.first & (cap - 1);
          while (tab[sl].count) sl = (sl + 1) & (cap - 1);
          tab[sl] = CountSlot{kv.first, kv.second.second};
        }
        HIP_TRY(cslots[k].ensure(cap));
        HIP_TRY(hipMemcpy(cslots[k].p, tab.data(), cap * sizeof(CountSlot), hipMemcpyHostToDevice));
        cmask[k] = cap - 1;
        small[k] = true;
      }
    }
    stamp("small marginals");
  }
  for (int k = 0; k < 2; ++k)
    if (!small[k]) HIP_TRY(rec[k].ensure(n));
  if (!rec_done && (!small[0] || !small[1])) {
    hipLaunchKernelGGL(freq_project2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, joint->stream,
                       joint->compact.p, n, arena_of(joint), part_types(joint, 1),
                       small[0] ? nullptr : rec[0].p, small[1] ? nullptr : rec[1].p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(joint->stream));
  }
  stamp("project");
  bool by_hash = !force_lookup;  // no marginal has two keys on one 64-bit hash
  for (int k = 0; k < 2 && res == DQ_OK; ++k) {
    if (small[k]) continue;
    const int32_t ty = joint->types[k];
    res = dq_freq_create(joint->device, 1, &ty, 0, &marg[k]);
    stamp(k ? "marginal 1 create" : "marginal 0 create");
    if (res == DQ_OK) {
      const int64_t rc[1] = {n};
      const int64_t vb[1] = {(int64_t)((joint->arena_used + 7) & ~7ULL)};
      const int64_t special[3] = {0, 0, (int64_t)joint->h_counters[C_NULL_ROWS]};
      res = add_records(marg[k], reinterpret_cast<const dq_freq_record*>(rec[k].p), arena_of(joint), 1, rc,
                        vb, joint->num_rows, special, 0, hip_stream, !marg[k]->exact);
    }
    stamp(k ? "marginal 1 records" : "marginal 0 records");
    // statistics first: the entropy identity below may make the groups unnecessary
    if (res == DQ_OK) res = finalize_c(marg[k], false, false);
    stamp(k ? "marginal 1 statistics" : "marginal 0 statistics");
    if (res != DQ_OK) break;
    if (marg[k]->h_counters[C_COLLISIONS]) by_hash = false;
  }
  // MI = E(X) + E(Y) - E(X, Y), every entropy normalised by the same numRows as the reference's
  // terms ((pxy/n) ln((pxy/n) / ((px/n)(py/n))) summed over the joint groups, the marginals
  // summed over them too: MutualInformation.scala:41-75) -- exact algebra over the fixed-point
  // sums of the tables' own -p ln p terms (the joint's and a general side's from phase C, a small
  // side's from its value counts with the same device term).  Taken when MI >= 1/100 of
  // E(X) + E(Y) + E(X, Y): each entropy's rounding is then below 1e-13 of MI (two columns close
  // to independent keep the per-group terms, whose sum does not cancel).
  if (res == DQ_OK) {
    fix128 ex[2];
    for (int k = 0; k < 2 && res == DQ_OK; ++k) {
      if (!small[k]) {
        ex[k] = marg[k]->st_entropy_fix;
        continue;
      }
      DevBuf<unsigned long long> acc;
      unsigned long long w[2];
      if (acc.ensure(2) != hipSuccess || hipMemsetAsync(acc.p, 0, 16, stream) != hipSuccess) {
        res = fail(DQ_ERR_OUT_OF_MEMORY, "MutualInformation entropy");
        break;
      }
      hipLaunchKernelGGL(freq_slots_entropy, dim3(1), dim3(256), 0, stream, cslots[k].p, cmask[k] + 1,
                         (double)joint->num_rows, acc.p);
      if (hipGetLastError() != hipSuccess || d2h(w, acc.p, 16, stream) != hipSuccess) {
        res = fail(DQ_ERR_DEVICE, "MutualInformation entropy");
        break;
      }
      ex[k] = (fix128)(((unsigned __int128)w[1] << 64) | w[0]);
    }
    if (res == DQ_OK) {
      const fix128 exy = joint->st_entropy_fix, v = ex[0] + ex[1] - exy;
      if (v > 0 && v * 100 >= ex[0] + ex[1] + exy) {
        *mi = fix_to_f64(v);
        for (int k = 0; k < 2; ++k)
          if (marg[k]) dq_freq_destroy(marg[k]);
        stamp("entropy identity");
        return DQ_OK;
      }
    }
  }
  for (int k = 0; k < 2 && res == DQ_OK; ++k) {  // the per-group terms: each general side's groups
    if (small[k]) continue;
    // (the groups stay where phase C put them, per partition; compacted only for the
    // byte-compare lookups)
    res = finalize_c(marg[k], true, false);
    stamp(k ? "marginal 1 groups" : "marginal 0 groups");
  }
  if (res == DQ_OK && !by_hash && (small[0] || small[1])) {
    // a general side counted a hash collision: the byte-compare lookups need both sides as
    // tables, so the small sides are built the general way too
    for (int k = 0; k < 2 && res == DQ_OK; ++k) {
      if (!small[k]) continue;
      small[k] = false;
      if (rec[k].ensure(n) != hipSuccess) {
        res = fail(DQ_ERR_OUT_OF_MEMORY, "MutualInformation records");
        break;
      }
      hipLaunchKernelGGL(freq_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, joint->stream,
                         joint->compact.p, n, arena_of(joint), part_types(joint, 1), k, rec[k].p);
      const int32_t ty = joint->types[k];
      res = dq_freq_create(joint->device, 1, &ty, 0, &marg[k]);
      if (res == DQ_OK) {
        const int64_t rc[1] = {n};
        const int64_t vb[1] = {(int64_t)((joint->arena_used + 7) & ~7ULL)};
        const int64_t special[3] = {0, 0, (int64_t)joint->h_counters[C_NULL_ROWS]};
        res = add_records(marg[k], reinterpret_cast<const dq_freq_record*>(rec[k].p), arena_of(joint), 1,
                          rc, vb, joint->num_rows, special, 0, hip_stream, !marg[k]->exact);
      }
      if (res == DQ_OK) res = compact_groups(marg[k]);
    }
  }
  CountIndex X[2];
  DevBuf<unsigned long long> pbase[2];
  DevBuf<uint8_t> plog[2];
  for (int k = 0; k < 2; ++k) X[k] = CountIndex{cslots[k].p, cmask[k], nullptr, nullptr, 0};
  for (int k = 0; k < 2 && res == DQ_OK; ++k) {
    if (small[k]) continue;
    const int32_t ty = joint->types[k];
    if (by_hash) {  // per partition, in LDS, when every partition's table fits
      dq_freq* mg = marg[k];
      const int64_t P = (int64_t)kBuckets << mg->s_bits;
      std::vector<unsigned long long> cnt(P), base(P);
      std::vector<uint8_t> lg(P);
      if (d2h(cnt.data(), mg->part_groups.p, P * 8, mg->stream) != hipSuccess) {
        res = fail(DQ_ERR_DEVICE, "marginal index");
        break;
      }
      unsigned long long tot = 0;
      bool fits = true;
      for (int64_t q = 0; q < P; ++q) {
        int l = 4;
        while ((1ULL << l) < 2 * cnt[q]) ++l;
        fits = fits && l <= kIdxMaxLog;
        lg[q] = (uint8_t)l;
        base[q] = tot;
        tot += 1ULL << l;
      }
      if (fits) {
        if (cslots[k].ensure(tot) != hipSuccess || pbase[k].ensure(P) != hipSuccess ||
            plog[k].ensure(P) != hipSuccess ||
            hipMemcpy(pbase[k].p, base.data(), P * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(plog[k].p, lg.data(), P, hipMemcpyHostToDevice) != hipSuccess) {
          res = fail(DQ_ERR_OUT_OF_MEMORY, "marginal index");
          break;
        }
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, joint->device);
        hipLaunchKernelGGL(freq_count_index_parts, dim3((unsigned)std::min<int64_t>(P, 2 * cus)), dim3(256), 0,
                           mg->stream, mg->groups.p, mg->part_off.p, mg->part_groups.p, P, pbase[k].p,
                           plog[k].p, cslots[k].p);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(mg->stream) != hipSuccess) {
          res = fail(DQ_ERR_DEVICE, "marginal index");
          break;
        }
        X[k] = CountIndex{cslots[k].p, 0, pbase[k].p, plog[k].p, 64 - kBucketBits - mg->s_bits};
      } else {  // one table over the compacted groups
        res = compact_groups(mg);
        if (res != DQ_OK) break;
        const int64_t m = mg->n_compact;
        uint64_t cap = 2;
        while (cap < (uint64_t)(2 * m)) cap <<= 1;
        if (cslots[k].ensure(cap) != hipSuccess ||
            hipMemsetAsync(cslots[k].p, 0, cap * sizeof(CountSlot), stream) != hipSuccess) {
          res = fail(DQ_ERR_OUT_OF_MEMORY, "marginal index");
          break;
        }
        if (m)
          hipLaunchKernelGGL(freq_count_index, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream,
                             mg->compact.p, m, cap - 1, cslots[k].p);
        X[k] = CountIndex{cslots[k].p, cap - 1, nullptr, nullptr, 0};
      }
    } else {
      res = compact_groups(marg[k]);
      if (res != DQ_OK) break;
      const int64_t m = marg[k]->n_compact;
      uint64_t cap = 2;
      while (cap < (uint64_t)(2 * m)) cap <<= 1;
      if (slots[k].ensure(cap) != hipSuccess || hipMemsetAsync(slots[k].p, 0, cap * 4, stream) != hipSuccess) {
        res = fail(DQ_ERR_OUT_OF_MEMORY, "marginal index");
        break;
      }
      if (m)
        hipLaunchKernelGGL(freq_lookup_build, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream,
                           marg[k]->compact.p, m, cap - 1, slots[k].p);
      L[k] = Lookup{marg[k]->compact.p, slots[k].p, cap - 1, arena_of(marg[k]), ty, marg[k]->exact ? 1 : 0,
                    marg[k]->rec_var_base};
    }
    stamp(k ? "marginal 1 index" : "marginal 0 index");
  }
  if (res == DQ_OK) {
    DevBuf<double> terms;
    DevBuf<unsigned long long> partial;
    constexpr int kSumBlocks = 1024;
    if (terms.ensure(n) != hipSuccess || partial.ensure(3 * kSumBlocks) != hipSuccess) {
      res = fail(DQ_ERR_OUT_OF_MEMORY, "MutualInformation terms");
    } else {
      if (by_hash) {
        const uint64_t* kp[2];
        int kst[2], kex[2];
        for (int k = 0; k < 2; ++k) {
          kp[k] = small[k] ? reinterpret_cast<const uint64_t*>(hk[k].p) : reinterpret_cast<const uint64_t*>(rec[k].p);
          kst[k] = small[k] ? 1 : (int)(sizeof(RecIn) / 8);
          kex[k] = small[k] ? 0 : (marg[k]->exact ? 1 : 0);
        }
        hipLaunchKernelGGL(freq_mi_terms_h, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           joint->compact.p, n, kp[0], kst[0], kp[1], kst[1], kex[0], kex[1], X[0], X[1],
                           (double)joint->num_rows, terms.p);
      } else {
        hipLaunchKernelGGL(freq_mi_terms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           joint->compact.p, n, arena_of(joint), part_types(joint, 1), L[0], L[1],
                           (double)joint->num_rows, terms.p);
      }
      stamp("terms");
      hipLaunchKernelGGL(freq_sum_fix, dim3(kSumBlocks), dim3(256), 0, stream, terms.p, n, partial.p);
      std::vector<unsigned long long> h(3 * kSumBlocks);
      if (hipGetLastError() != hipSuccess ||
          d2h(h.data(), partial.p, 3 * kSumBlocks * 8, stream) != hipSuccess) {
        res = fail(DQ_ERR_DEVICE, "MutualInformation launch failed");
      } else {
        fix128 sum = 0;
        double nf = 0.0;
        for (int b = 0; b < kSumBlocks; ++b) {
          sum += (fix128)(((unsigned __int128)h[3 * b + 1] << 64) | h[3 * b]);
          nf += __builtin_bit_cast(double, h[3 * b + 2]);
        }
        *mi = fix_to_f64(sum) + nf;
      }
    }
  }
  stamp("sum");
  for (dq_freq* m : marg) dq_freq_destroy(m);
  stamp("destroy");
  return res;
}
