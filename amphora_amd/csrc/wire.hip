// The fused wire-format kernels: K_RV / K_MASK straight from the base64 text
// of the ODO fields (getSecret / createSecret with Jackson's base64 decode of
// every byte[] field, DefaultAmphoraClient.java:150-170,206-217): the text is
// decoded in the workgroup and consumed through LDS.  Bound: the decode's
// integer VALU work ("Wire kernels, round 4": a register form
// without LDS, a persistent software-pipelined form and an occupancy sweep
// were measured and rejected -- tools/ubench/ubench_wire_occ.hip).
#include <cstdlib>
#include <string>

#include "b64.hpp"
#include "bodyspans.hpp"
#include "devio.hpp"
#include "wiretiles.hpp"

namespace amph {
namespace {

// ---- fused wire-format kernels ----------------------------------------------
// The client receives each party's ODO as base64 text (VerifiableSecretShare /
// OutputDeliveryObject JSON, Jackson's Base64Variants.MIME_NO_LINEFEEDS) and
// sends each masked word as a 24-character record (MaskedInputData).  Decoding
// the 5N fields to HBM and then running K_RV / K_MASK moves 4/3 x 80N + 2 x 80N
// bytes per word; these kernels decode the text in the workgroup and consume
// it from LDS, so the decoded words never reach HBM (K_RV from text: 4/3 x
// 80N + 16 B/word).
//
// A workgroup of kWireBlock lanes owns 16 x kWireBlock characters of every
// field = 12 x kWireBlock bytes = kWireWords words.  Per field every lane
// decodes one 16-character unit (4 groups) and writes its 12 bytes to LDS;
// after a barrier the first kWireWords lanes (whole waves: the last quarter of
// the waves only decode) read their 16-byte word and add it into the field's
// sum.  Two LDS buffers alternate, so one barrier per field suffices.  The
// text's final group may carry '=' padding: the workgroup that holds it
// (or any character past the text) takes the per-character path.
constexpr int kWireBlock = 256;  // workgroup size: 256 > 512 > 1024 by 15-50 % (tools/ubench/ubench_wire.hip)
template <int BS>
struct Wire {
  static constexpr int words = BS * 3 / 4;          // words per workgroup
  static constexpr size_t chars = (size_t)16 * BS;  // characters per field per workgroup
};

// One 16-character unit of a field's text, checked character by character:
// positions >= nchars decode as 'A' (zero bits, beyond the last word);
// the final `pad` positions must be '=' (decoded as 'A'), '=' anywhere else
// is invalid like any non-alphabet character.  Returns the unit's first
// invalid offset (or 0xFFFFFFFF) and its 12 bytes in o.
__device__ __forceinline__ uint32_t dec_unit_slow(const char* t, size_t unit, size_t nchars,
                                                  uint32_t pad, uint32_t (&o)[3]) {
  uint32_t w[4] = {0, 0, 0, 0}, forced = 0xFFFFFFFFu;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const size_t pos = 16 * unit + q;
    uint32_t ch = pos < nchars ? (uint8_t)t[pos] : (uint32_t)'A';
    if (pos < nchars && pos + pad >= nchars) {
      if (ch != '=' && forced == 0xFFFFFFFFu) forced = q;
      ch = 'A';
    }
    w[q >> 2] |= ch << (8 * (q & 3));
  }
  const uint32_t fb = dec_unit16(make_uint4(w[0], w[1], w[2], w[3]), o);
  return min(fb, forced);
}

// Sum field k over the parties from the text, consuming it through LDS.  raw:
// this lane's units, loaded up front on the fast path (FAST).
// Fast-path loads: kWirePrefetch > 0 issues field f + kWirePrefetch's load
// while field f is decoded (fewer live VGPRs); 0 issues all 5N up front.
#ifndef AMPH_WIRE_PD
#define AMPH_WIRE_PD 3  // with the LDS-table decode: 73-77 VGPRs at 3 parties (0: 99-101)
#endif
constexpr int kWirePrefetch = AMPH_WIRE_PD;

// Fields decoded per barrier (AMPH_WIRE_G): G units of text go to LDS before
// each barrier (2G buffers alternate, or all 5N at once, one barrier in all,
// when G >= 5N).
#ifndef AMPH_WIRE_G
// 3: 6 buffers + the 256-byte decode table = 18.7 KB per block, so LDS allows
// 6 waves per SIMD as the VGPRs do (G = 5: 30.3 KB, 5 waves); k_mask_b64
// -5 % at 4 Mi x 3 (profiles/r05_wire_lut_ab.txt).  r02: G = 5 was 2-5 % over 1.
#define AMPH_WIRE_G 3
#endif
template <int NP>
struct WireGroups {
  static constexpr int F = 5 * (NP > 0 ? NP : 1);  // fields (runtime party counts: G = 1)
  static constexpr int G = NP > 0 ? (AMPH_WIRE_G < F ? AMPH_WIRE_G : F) : 1;
  static constexpr int bufs = G >= F ? F : 2 * G;
};

// A fast-path unit with a bad character (rare): locate the first one and
// report (party j, field k) in ODO order, then the offset -- the same
// atomicMin the per-character path makes.
__device__ __forceinline__ void bad_unit(const uint4 v, int j, int k, size_t nchars, size_t unit,
                                         unsigned long long* bad) {
  uint32_t o[3];
  const uint32_t fb = dec_unit16(v, o);
  atomicMin(bad, (unsigned long long)((size_t)(5 * j + k) * nchars + 16 * unit + fb));
}

// The per-character path of one unit with its report (party j, field k in
// ODO order, then the offset).
__device__ __forceinline__ void slow_unit(const char* t, size_t unit, size_t nchars, uint32_t pad, int j, int k,
                                          uint32_t (&o)[3], unsigned long long* bad) {
  const uint32_t fb = dec_unit_slow(t, unit, nchars, pad, o);
  if (fb != 0xFFFFFFFFu)
    atomicMin(bad, (unsigned long long)((size_t)(5 * j + k) * nchars + 16 * unit + fb));
}

// One fast-path unit of a text: its 16 characters as four dwords.  BODY (the
// any-alignment form of k_acc_b64, include/amphora_client_bodies.h): the text
// starts at ANY byte of a 16-byte aligned buffer.  Two fetches, A/B on one
// MI355X at 4 Mi words x 3 parties (profiles/
// clients_bodies.json; three party launches, K = 1 / 64 / 1,024):
//   AMPH_BODY_FETCH = 1 (built): one 16-byte load at the text's own alignment,
//     exactly the unit's bytes -- 0.646 / 0.646 / 0.670 ms;
//   AMPH_BODY_FETCH = 0: the unit funnelled out of the one or two aligned
//     16-byte granules bodyspans.hpp names for it -- two loads per lane, the
//     second only when the unit straddles (its granule then holds the unit's
//     own last characters, so no granule without text is read); the residue is
//     the same for every unit of a text (workgroup-uniform), so the dword
//     selection is a scalar branch and v_alignbyte does the remaining 0-3
//     bytes -- 0.737 / 0.746 / 0.829 ms.
// (One load per lane plus the neighbour's through a cross-lane move was not
// built.)  Either way every byte read lies in a granule body_granules names.
#ifndef AMPH_BODY_FETCH
#define AMPH_BODY_FETCH 1
#endif
__device__ __forceinline__ uint4 funnel16(const uint4 lo, const uint4 hi, uint32_t residue) {
  const uint32_t a = __builtin_amdgcn_readfirstlane(residue), b = a & 3u;
  uint32_t s0, s1, s2, s3, s4;
  switch (a >> 2) {
    case 0: s0 = lo.x, s1 = lo.y, s2 = lo.z, s3 = lo.w, s4 = hi.x; break;
    case 1: s0 = lo.y, s1 = lo.z, s2 = lo.w, s3 = hi.x, s4 = hi.y; break;
    case 2: s0 = lo.z, s1 = lo.w, s2 = hi.x, s3 = hi.y, s4 = hi.z; break;
    default: s0 = lo.w, s1 = hi.x, s2 = hi.y, s3 = hi.z, s4 = hi.w; break;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(s1, s0, b), __builtin_amdgcn_alignbyte(s2, s1, b),
                    __builtin_amdgcn_alignbyte(s3, s2, b), __builtin_amdgcn_alignbyte(s4, s3, b));
}

template <bool BODY>
__device__ __forceinline__ uint4 text_unit(const char* t, size_t unit, size_t nchars) {
  if constexpr (!BODY) {
    return ld(reinterpret_cast<const uint4*>(t) + unit);
  } else if constexpr (AMPH_BODY_FETCH == 1) {
    typedef unsigned int bu32x4 __attribute__((ext_vector_type(4), aligned(1)));
    const bu32x4 v = *reinterpret_cast<const bu32x4*>(t + 16 * unit);
    return make_uint4(v.x, v.y, v.z, v.w);
  } else {
    const BodyUnit bu = body_unit((uint64_t)(uintptr_t)t, nchars, unit);
    const uint4* g = reinterpret_cast<const uint4*>((uintptr_t)(bu.first << 4));
    const uint4 lo = ld(g);
    uint4 hi = lo;
    if (bu.n == 2) hi = ld(g + 1);
    return funnel16(lo, hi, bu.residue);
  }
}

// toff: the texts start this many characters (a multiple of 16) into every
// field buffer (the segmented kernels' slot offset).  MIXED (with FAST): the
// tile that holds a text's end, lane by lane -- a lane whose unit ends at
// least 4 characters before nchars (lane_fast) loads and decodes as the fast
// path does, a lane whose unit starts at or past nchars contributes zero
// bits (what the per-character path decodes there) without decoding, and the
// one or two lanes in between take the per-character path and read nothing
// past the text.  BODY: text_unit's any-alignment fetch (the pointers of tx are
// then the texts' own first bytes, toff 0); the per-character path reads byte
// by byte at any address as it is.
template <int NP, bool BIG, bool FAST, int BS, bool MIXED = false, bool BODY = false>
__device__ __forceinline__ void wire_fields(const TextSet& tx, int n, size_t nchars, uint32_t pad,
                                            size_t words, uint4 (&raw)[5][NP > 0 ? NP : 1],
                                            uint32_t (*lds)[3 * BS], W4 (&acc)[5],
                                            unsigned long long* bad, const Fp& f, size_t tile,
                                            const uint8_t* lutp, size_t toff = 0, bool lane_fast = true) {
  constexpr int G = WireGroups<NP>::G, NB = WireGroups<NP>::bufs;
  const size_t unit = tile * BS + threadIdx.x;
  const size_t word = tile * Wire<BS>::words + threadIdx.x;
  const bool consumer = threadIdx.x < Wire<BS>::words && word < words;
  const bool lane_past = MIXED && 16 * unit >= nchars;  // the whole unit lies past the text: zero bits
  const int np = NP > 0 ? NP : n;
  int slot = 0;  // LDS buffer of the next field
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int j = 0; j < (NP > 0 ? NP : kMaxParties); ++j) {
      if (NP == 0 && j >= np) break;
      uint32_t o[3];
      if constexpr (FAST && NP > 0) {
        if constexpr (kWirePrefetch > 0) {
          const int ahead = k * NP + j + kWirePrefetch;
          if (ahead < 5 * NP && (!MIXED || lane_fast))
            raw[ahead / NP][ahead % NP] = text_unit<BODY>(tx.t[ahead / NP][ahead % NP] + toff, unit, nchars);
        }
        if (!MIXED || lane_fast) {
          uint32_t badb = 0;  // the per-unit branch also bounds the LDS reads' live ranges: one
          dec_unit16_lut(raw[k][j], o, badb, lutp);  // check after the last field took 117-256 VGPRs
          if (badb & 0x80u) bad_unit(raw[k][j], j, k, nchars, unit, bad);
        } else if (lane_past) {
          o[0] = o[1] = o[2] = 0;
        } else {
          slow_unit(tx.t[k][j] + toff, unit, nchars, pad, j, k, o, bad);
        }
      } else if constexpr (FAST) {
        if (!MIXED || lane_fast) {
          const uint4 v = text_unit<BODY>(tx.t[k][j] + toff, unit, nchars);
          uint32_t badb = 0;
          dec_unit16_lut(v, o, badb, lutp);
          if (badb & 0x80u) bad_unit(v, j, k, nchars, unit, bad);
        } else if (lane_past) {
          o[0] = o[1] = o[2] = 0;
        } else {
          slow_unit(tx.t[k][j] + toff, unit, nchars, pad, j, k, o, bad);
        }
      } else {
        slow_unit(tx.t[k][j] + toff, unit, nchars, pad, j, k, o, bad);
      }
      uint32_t* l = lds[slot];
      l[3 * threadIdx.x] = o[0];
      l[3 * threadIdx.x + 1] = o[1];
      l[3 * threadIdx.x + 2] = o[2];
      const int fi = k * (NP > 0 ? NP : 1) + j;  // flat field index (G = 1 for runtime counts)
      const bool group_end = G == 1 || (fi + 1) % G == 0 || fi + 1 == WireGroups<NP>::F;
      if (group_end) {
        __syncthreads();
        if (consumer) {
          // the group's fields, oldest first: fields fi - m, m = cnt-1 .. 0
          const int cnt = G == 1 ? 1 : (fi % G) + 1;
#pragma unroll
          for (int m = (G == 1 ? 0 : G - 1); m >= 0; --m) {
            if (m >= cnt) continue;
            const int ff = fi - m, kk = G == 1 ? k : ff / (NP > 0 ? NP : 1), jj = G == 1 ? j : ff % (NP > 0 ? NP : 1);
            const int sl = (slot - m + NB) % NB;
            const uint4 v = reinterpret_cast<const uint4*>(lds[sl])[threadIdx.x];
            const W4 x = canon<BIG>(w4(v), f);
            acc[kk] = jj == 0 ? x : mod_add(acc[kk], x, f);
          }
        }
      }
      slot = (slot + 1) % NB;
    }
  }
}

template <int NP, int BS, bool BODY = false>
__device__ __forceinline__ void wire_load(const TextSet& tx, uint4 (&raw)[5][NP > 0 ? NP : 1], size_t tile,
                                          size_t toff = 0, bool lane_fast = true, size_t nchars = 0) {
  if constexpr (NP > 0) {
    const size_t unit = tile * BS + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if ((kWirePrefetch == 0 || k * NP + j < kWirePrefetch) && lane_fast)
          raw[k][j] = text_unit<BODY>(tx.t[k][j] + toff, unit, nchars);
  }
}

// The framed form of the records: the "data" array text of the MaskedInput
// body as Jackson writes it (MaskedInput.java:25-62, MaskedInputData.java:
// 44-52), '[' + {"value":"<24 chars>"} per secret, ',' between, ']'.
constexpr int kJsonRec = 37;  // bytes per record, its ',' / ']' included

// K_MASK from the wire, after a tile's fields are summed: verify, mask the
// secret, and write the masked word and / or its 24-character record (each
// lane its own, as three nontemporal 8-byte stores).
//
// JSON: out24 is the framed text instead.  The workgroup owns the 37 WW
// bytes (a whole number of 16-byte runs) from the ',' / '[' in front of its
// first record on; the workgroup of the last secret also owns the ']'.  The
// image is built in LDS (lds: the decode buffers, free after a barrier) --
// each lane writes the aligned dwords that START inside its record, whose
// bytes past the record are the next record's constant {"v -- and leaves as
// coalesced nontemporal 16-byte runs; the text's final partial run byte by
// byte, so nothing past the ']' is written.
template <int NP, int BS, bool JSON = false>
__device__ __forceinline__ void mask_tile_out(size_t tile, size_t words, const uint4 s, size_t n_secrets,
                                              W4 (&acc)[5], uint4* out16, char* out24,
                                              unsigned long long* ff, uint32_t (*lds)[3 * BS], const Fp& f) {
  constexpr int WW = Wire<BS>::words;
  const size_t word = tile * WW + threadIdx.x;
  const bool has_secret = threadIdx.x < WW && word < n_secrets;
  uint32_t g[6];
  if (threadIdx.x < WW) {
    const bool in = word < words;
    bool ok = true;
    if (in) ok = (int)eq(mont_mul_v(acc[0], acc[1], f), acc[3]) & (int)eq(mont_mul_v(acc[2], acc[1], f), acc[4]);
    report_fail(in && !ok, word, ff);
    if (has_secret) {
      const uint4 m = u4(mod_sub(mont_mul_v(w4(s), r2_word(f), f), acc[0], f));
      if (!JSON && out16) st_out(out16 + word, w4(m));
      enc_word24(m, g);
    }
  }
  if constexpr (JSON) {
    static_assert((kJsonRec * WW) % 16 == 0, "a workgroup's records are whole 16-byte runs");
    const size_t r0 = tile * WW;
    if (r0 >= n_secrets) return;  // (the whole workgroup)
    const uint32_t nrec = (uint32_t)min((size_t)WW, n_secrets - r0);
    const uint32_t total = kJsonRec * nrec + (r0 + nrec == n_secrets ? 1u : 0u);
    uint32_t* img = &lds[0][0];
    __syncthreads();  // every lane is past its last read of the decode buffers
    if (has_secret) {
      constexpr uint32_t kOpen = 0x76227B00u;  // {"v in bytes 1-3
      const uint32_t r[10] = {0x6176227Bu, 0x2265756Cu, 0x223Au | (g[0] << 16),
                              (g[0] >> 16) | (g[1] << 16), (g[1] >> 16) | (g[2] << 16),
                              (g[2] >> 16) | (g[3] << 16), (g[3] >> 16) | (g[4] << 16),
                              (g[4] >> 16) | (g[5] << 16), (g[5] >> 16) | 0x7D220000u,
                              (word + 1 == n_secrets ? (uint32_t)']' : (uint32_t)',') | kOpen};
      const uint32_t o = 1 + kJsonRec * threadIdx.x, e = (4 - (o & 3)) & 3, base = (o + 3) >> 2;
#pragma unroll
      for (int j = 0; j < 9; ++j) img[base + j] = __builtin_amdgcn_alignbyte(r[j + 1], r[j], e);
      if (e == 0) img[base + 9] = r[9];
      if (threadIdx.x == 0) img[0] = (tile == 0 ? (uint32_t)'[' : (uint32_t)',') | kOpen;
    }
    __syncthreads();
    char* dst = out24 + (size_t)kJsonRec * r0;
    typedef unsigned int ju32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t q = threadIdx.x; q < total / 16; q += BS)
      __builtin_nontemporal_store(reinterpret_cast<const ju32x4*>(img)[q], reinterpret_cast<ju32x4*>(dst) + q);
    const uint32_t done = total & ~15u;
    if (threadIdx.x < total - done) dst[done + threadIdx.x] = reinterpret_cast<const char*>(img)[done + threadIdx.x];
    return;
  }
  if (!out24 || !has_secret) return;
  // records: each lane streams its own 24 bytes as three nontemporal 8-byte
  // stores; a wave's three store instructions cover its 1536 contiguous
  // bytes, which the L2 merges into whole lines.  Round 5 staged the
  // workgroup's records in LDS and stored 16-byte runs behind two barriers:
  // sustained k_mask_b64 277.8 -> 265.6 us at 4 Mi x 3 (plain 8-byte stores:
  // 274.2), 0.95-0.96 of its access-pattern probe
  // (profiles/r06_wire_record_stores_ab.txt)
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  u32x2* o = reinterpret_cast<u32x2*>(out24 + 24 * word);
  __builtin_nontemporal_store(u32x2{g[0], g[1]}, o);
  __builtin_nontemporal_store(u32x2{g[2], g[3]}, o + 1);
  __builtin_nontemporal_store(u32x2{g[4], g[5]}, o + 2);
}

// Waves per SIMD the register allocation must allow (0: the compiler's choice;
// tools/ubench A/B knob, spills below ~96 VGPRs).
#ifndef AMPH_WIRE_WPE
#define AMPH_WIRE_WPE 0
#endif
#if AMPH_WIRE_WPE > 0
#define AMPH_WIRE_OCC __attribute__((amdgpu_waves_per_eu(AMPH_WIRE_WPE)))
#else
#define AMPH_WIRE_OCC
#endif

// K_RV from the wire: the N parties' base64 ODO fields -> canonical secrets,
// MAC verify (getSecret, DefaultAmphoraClient.java:206-217 incl. the Jackson
// base64 decode of every field).  bad: min (5 party + field) * nchars + offset
// of an invalid character.
template <int NP, bool BIG, int BS>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_rv_b64(TextSet tx, int n, size_t words, size_t nchars,
                                           uint32_t pad, uint4* out_y, unsigned long long* ff,
                                           unsigned long long* bad, Fp f) {
  __shared__ uint32_t lds[WireGroups<NP>::bufs < 2 ? 2 : WireGroups<NP>::bufs][3 * BS];
  __shared__ uint32_t lutw[kLutBytes / 4];
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  b64_lut_fill(lutp);
  __syncthreads();
  W4 acc[5];
  uint4 raw[5][NP > 0 ? NP : 1];
  const bool fast = ((size_t)blockIdx.x + 1) * Wire<BS>::chars + 4 <= nchars;
  if (fast) {
    wire_load<NP, BS>(tx, raw, blockIdx.x);
    wire_fields<NP, BIG, true, BS>(tx, n, nchars, pad, words, raw, lds, acc, bad, f, blockIdx.x, lutp);
  } else {
    wire_fields<NP, BIG, false, BS>(tx, n, nchars, pad, words, raw, lds, acc, bad, f, blockIdx.x, lutp);
  }
  const size_t word = (size_t)blockIdx.x * Wire<BS>::words + threadIdx.x;
  if (threadIdx.x < Wire<BS>::words) {  // whole waves
    const bool in = word < words;
    bool ok = true;
    if (in) {
      ok = (int)eq(mont_mul_v(acc[0], acc[1], f), acc[3]) & (int)eq(mont_mul_v(acc[2], acc[1], f), acc[4]);
      st_out(out_y + word, redc(acc[0], f));
    }
    report_fail(in && !ok, word, ff);
  }
}

// K_MASK from the wire: the N parties' base64 Input Mask ODO fields + the
// secrets -> verify the masks, masked[i] = toGfp((s_i - m_i) mod p) for
// i < n_secrets, written as raw words (out16) and/or as the 24-character
// base64 records of MaskedInputData (out24, each lane its own record as three
// nontemporal 8-byte stores).  createSecret, DefaultAmphoraClient.java:150-170.
template <int NP, bool BIG, int BS>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_mask_b64(TextSet tx, int n, size_t words, size_t nchars,
                                             uint32_t pad, const uint4* secrets, size_t n_secrets,
                                             uint4* out16, char* out24, unsigned long long* ff,
                                             unsigned long long* bad, Fp f) {
  constexpr int WW = Wire<BS>::words;
  __shared__ uint32_t lds[WireGroups<NP>::bufs < 2 ? 2 : WireGroups<NP>::bufs][3 * BS];
  __shared__ uint32_t lutw[kLutBytes / 4];
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  b64_lut_fill(lutp);
  __syncthreads();
  W4 acc[5];
  uint4 raw[5][NP > 0 ? NP : 1];
  const size_t word = (size_t)blockIdx.x * WW + threadIdx.x;
  const bool has_secret = threadIdx.x < WW && word < n_secrets;
  const bool fast = ((size_t)blockIdx.x + 1) * Wire<BS>::chars + 4 <= nchars;
  if (fast) {
    wire_load<NP, BS>(tx, raw, blockIdx.x);
    wire_fields<NP, BIG, true, BS>(tx, n, nchars, pad, words, raw, lds, acc, bad, f, blockIdx.x, lutp);
  } else {
    wire_fields<NP, BIG, false, BS>(tx, n, nchars, pad, words, raw, lds, acc, bad, f, blockIdx.x, lutp);
  }
  // the secret after the decode: loaded up front it held 4 VGPRs through it
  // (98 VGPRs: 4 waves per SIMD instead of 5); the other waves hide its latency
  uint4 s = make_uint4(0, 0, 0, 0);
  if (has_secret) s = ld(secrets + word);
  mask_tile_out<NP, BS>(blockIdx.x, words, s, n_secrets, acc, out16, out24, ff, lds, f);
}

// k_mask_b64 with the masked words written as the framed "data" array text
// of the MaskedInput body (mask_tile_out's JSON form): out_text, 16-byte
// aligned, gets 37 n_secrets + 1 characters (n_secrets >= 1).
template <int NP, bool BIG, int BS>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_mask_json(TextSet tx, int n, size_t words, size_t nchars,
                                              uint32_t pad, const uint4* secrets, size_t n_secrets,
                                              char* out_text, unsigned long long* ff,
                                              unsigned long long* bad, Fp f) {
  constexpr int WW = Wire<BS>::words;
  // (at least 3 buffers: the text image of WW records needs 37 WW + 4 bytes)
  __shared__ __attribute__((aligned(16))) uint32_t lds[WireGroups<NP>::bufs < 3 ? 3 : WireGroups<NP>::bufs][3 * BS];
  static_assert(3 * 3 * BS * 4 >= kJsonRec * WW + 4, "the text image fits the decode buffers");
  __shared__ uint32_t lutw[kLutBytes / 4];
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  b64_lut_fill(lutp);
  __syncthreads();
  W4 acc[5];
  uint4 raw[5][NP > 0 ? NP : 1];
  const size_t word = (size_t)blockIdx.x * WW + threadIdx.x;
  const bool has_secret = threadIdx.x < WW && word < n_secrets;
  const bool fast = ((size_t)blockIdx.x + 1) * Wire<BS>::chars + 4 <= nchars;
  if (fast) {
    wire_load<NP, BS>(tx, raw, blockIdx.x);
    wire_fields<NP, BIG, true, BS>(tx, n, nchars, pad, words, raw, lds, acc, bad, f, blockIdx.x, lutp);
  } else {
    wire_fields<NP, BIG, false, BS>(tx, n, nchars, pad, words, raw, lds, acc, bad, f, blockIdx.x, lutp);
  }
  uint4 s = make_uint4(0, 0, 0, 0);  // (after the decode, as k_mask_b64)
  if (has_secret) s = ld(secrets + word);
  mask_tile_out<NP, BS, true>(blockIdx.x, words, s, n_secrets, acc, nullptr, out_text, ff, lds, f);
}

// ---- many secrets per launch: the slotted text layout ---------------------------
// K objects' texts in one launch (include/amphora_wire_batch.h): every one of
// the 5N field buffers holds object o's own base64 text, its own '=' padding
// included, at character offset toff[o] (a multiple of 16, the same in every
// buffer); the objects' words are packed on woff[n_objects + 1] as in the
// packed word calls.  A workgroup decodes one tile of ONE object
// (wiretiles.hpp: which one, without a scan), so everything above applies with
// that object's nchars / pad / words, the text pointers advanced by its slot
// and the outputs by woff[o]; the verdict words are first_fail[o] / bad[o]
// with object-local indices -- bit for bit what the single call on that object
// alone reports.  Bytes of a buffer outside the texts are never read.
//
// The tile that holds a text's end is one per OBJECT here (1 in 6 at 1,000
// words, every tile below 192): AMPH_WIRE_SEG_LANES = 1 decodes it lane by
// lane (wire_fields' MIXED form: only the lanes that hold the final group
// take the per-character path, the divergence stays in one wave), 0 takes the
// whole tile through the per-character path as k_rv_b64 does (DESIGN.md
// section 4c', "the last tile").
#ifndef AMPH_WIRE_SEG_LANES
#define AMPH_WIRE_SEG_LANES 1
#endif

struct SegTile {
  size_t o, tile;  // the object and its tile
  size_t w0, words, nchars, toff;
  uint32_t pad;
};

// This workgroup's tile (wave-uniform: scalar loads only); false: none.  The
// word range is clamped into [0, woff[n_objects]], so whatever the table holds
// no output word past the packed arrays' T words is written.
template <int BS>
__device__ __forceinline__ bool seg_tile(const uint64_t* woff, const uint64_t* toff, size_t n_objects, SegTile& s) {
  static_assert(Wire<BS>::words == kWireTileWords, "wiretiles.hpp's tile is this workgroup's");
  const WireTile wt = wire_tile_find(woff, n_objects, blockIdx.x, Wire<BS>::words);
  const uint64_t T = woff[n_objects];
  const uint64_t a = woff[wt.object], b = woff[wt.object + 1];
  const uint64_t w0 = a < T ? a : T, w1 = b < w0 ? w0 : (b < T ? b : T);
  s.o = wt.object, s.tile = wt.local, s.w0 = w0, s.words = w1 - w0;  // (also of a workgroup without a tile)
  if (!wire_tile_real(wt.local, w1 - w0, Wire<BS>::words)) return false;
  s.nchars = wire_text_chars(s.words);
  s.pad = (uint32_t)((3 - (16 * s.words) % 3) % 3);
  s.toff = toff[wt.object];
  return true;
}

template <int NP, bool BIG, int BS, bool BODY = false>
__device__ __forceinline__ void seg_fields(const TextSet& tx, int n, const SegTile& s,
                                           uint4 (&raw)[5][NP > 0 ? NP : 1], uint32_t (*lds)[3 * BS],
                                           W4 (&acc)[5], unsigned long long* bad, const Fp& f,
                                           const uint8_t* lutp) {
  const bool fast = (s.tile + 1) * Wire<BS>::chars + 4 <= s.nchars;
  if (fast) {
    wire_load<NP, BS, BODY>(tx, raw, s.tile, s.toff, true, s.nchars);
    wire_fields<NP, BIG, true, BS, false, BODY>(tx, n, s.nchars, s.pad, s.words, raw, lds, acc, bad, f, s.tile, lutp,
                                                s.toff);
  } else if constexpr (AMPH_WIRE_SEG_LANES) {
    const bool lane_fast = 16 * (s.tile * BS + threadIdx.x + 1) + 4 <= s.nchars;
    wire_load<NP, BS, BODY>(tx, raw, s.tile, s.toff, lane_fast, s.nchars);
    wire_fields<NP, BIG, true, BS, true, BODY>(tx, n, s.nchars, s.pad, s.words, raw, lds, acc, bad, f, s.tile, lutp,
                                               s.toff, lane_fast);
  } else {
    wire_fields<NP, BIG, false, BS>(tx, n, s.nchars, s.pad, s.words, raw, lds, acc, bad, f, s.tile, lutp, s.toff);
  }
}

// k_rv_b64 over the slotted layout: out_y packed on woff, ff / bad arrays of
// n_objects words.
template <int NP, bool BIG, int BS>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_rv_b64_seg(TextSet tx, int n, const uint64_t* woff,
                                               const uint64_t* toff, size_t n_objects, uint4* out_y,
                                               unsigned long long* ff, unsigned long long* bad, Fp f) {
  __shared__ uint32_t lds[WireGroups<NP>::bufs < 2 ? 2 : WireGroups<NP>::bufs][3 * BS];
  __shared__ uint32_t lutw[kLutBytes / 4];
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  SegTile s;
  const bool real = seg_tile<BS>(woff, toff, n_objects, s);  // its table loads fly during the fill
  b64_lut_fill(lutp);
  __syncthreads();
  if (!real) return;  // (the whole workgroup)
  W4 acc[5];
  uint4 raw[5][NP > 0 ? NP : 1];
  seg_fields<NP, BIG, BS>(tx, n, s, raw, lds, acc, bad + s.o, f, lutp);
  const size_t word = s.tile * Wire<BS>::words + threadIdx.x;
  if (threadIdx.x < Wire<BS>::words) {  // whole waves
    const bool in = word < s.words;
    bool ok = true;
    if (in) {
      ok = (int)eq(mont_mul_v(acc[0], acc[1], f), acc[3]) & (int)eq(mont_mul_v(acc[2], acc[1], f), acc[4]);
      st_out(out_y + s.w0 + word, redc(acc[0], f));
    }
    report_fail(in && !ok, word, ff + s.o);
  }
}

// k_mask_b64 over the slotted layout: one secret per mask word, secrets /
// out16 / out24 packed on woff.
template <int NP, bool BIG, int BS>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_mask_b64_seg(TextSet tx, int n, const uint64_t* woff,
                                                 const uint64_t* toff, size_t n_objects, const uint4* secrets,
                                                 uint4* out16, char* out24, unsigned long long* ff,
                                                 unsigned long long* bad, Fp f) {
  constexpr int WW = Wire<BS>::words;
  __shared__ uint32_t lds[WireGroups<NP>::bufs < 2 ? 2 : WireGroups<NP>::bufs][3 * BS];
  __shared__ uint32_t lutw[kLutBytes / 4];
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  SegTile s;
  const bool real = seg_tile<BS>(woff, toff, n_objects, s);  // its table loads fly during the fill
  b64_lut_fill(lutp);
  __syncthreads();
  if (!real) return;  // (the whole workgroup)
  W4 acc[5];
  uint4 raw[5][NP > 0 ? NP : 1];
  seg_fields<NP, BIG, BS>(tx, n, s, raw, lds, acc, bad + s.o, f, lutp);
  const size_t word = s.tile * WW + threadIdx.x;
  uint4 sec = make_uint4(0, 0, 0, 0);  // (after the decode, as k_mask_b64)
  if (threadIdx.x < WW && word < s.words) sec = ld(secrets + s.w0 + word);
  mask_tile_out<NP, BS>(s.tile, s.words, sec, s.words, acc, out16 ? out16 + s.w0 : nullptr,
                        out24 ? out24 + 24 * s.w0 : nullptr, ff + s.o, lds, f);
}

// k_mask_b64_seg with every object's masked words written as its own framed
// "data" array text (mask_tile_out's JSON form, include/amphora_upload_batch.h):
// object o's text goes to out_text + ooff[o], ooff[o] a multiple of 16, so the
// image's 16-byte nontemporal runs stay aligned -- 37 x 192 is a multiple of
// 16, every tile's records are whole runs from the object's own start on.
// The '[' goes with the object's tile 0 and the ']' with its last record, the
// final partial run leaves byte by byte: nothing past an object's ']' is
// written.  An object of no words has no tile; its "[]" is written by
// workgroup g(o) = woff[o] / 192 + o, which is no other object's real tile
// (wiretiles.hpp).
template <int NP, bool BIG, int BS>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_mask_json_seg(TextSet tx, int n, const uint64_t* woff,
                                                  const uint64_t* toff, const uint64_t* ooff, size_t n_objects,
                                                  const uint4* secrets, char* out_text, unsigned long long* ff,
                                                  unsigned long long* bad, Fp f) {
  constexpr int WW = Wire<BS>::words;
  // (at least 3 buffers for the text image, as k_mask_json)
  __shared__ __attribute__((aligned(16))) uint32_t lds[WireGroups<NP>::bufs < 3 ? 3 : WireGroups<NP>::bufs][3 * BS];
  static_assert(3 * 3 * BS * 4 >= kJsonRec * WW + 4, "the text image fits the decode buffers");
  __shared__ uint32_t lutw[kLutBytes / 4];
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  SegTile s;
  const bool real = seg_tile<BS>(woff, toff, n_objects, s);  // its table loads fly during the fill
  char* dst = out_text + ooff[s.o];
  b64_lut_fill(lutp);
  __syncthreads();
  if (!real) {  // (the whole workgroup)
    if (s.words == 0 && s.tile == 0 && threadIdx.x < 2) dst[threadIdx.x] = threadIdx.x ? ']' : '[';
    return;
  }
  W4 acc[5];
  uint4 raw[5][NP > 0 ? NP : 1];
  seg_fields<NP, BIG, BS>(tx, n, s, raw, lds, acc, bad + s.o, f, lutp);
  const size_t word = s.tile * WW + threadIdx.x;
  uint4 sec = make_uint4(0, 0, 0, 0);  // (after the decode, as k_mask_b64)
  if (threadIdx.x < WW && word < s.words) sec = ld(secrets + s.w0 + word);
  mask_tile_out<NP, BS, true>(s.tile, s.words, sec, s.words, acc, nullptr, dst, ff + s.o, lds, f);
}

// ---- one party at a time: the client session's running sums ---------------------
// (include/amphora_client_session.h)  The parties' responses reach a client one
// by one; recombination is a sum mod p of canonical Montgomery words, so a
// running sum per field is exact in any arrival order.  k_acc_b64 decodes ONE
// party's five texts exactly as k_rv_b64 does for a single party (the same
// tile, fast / per-character split and LDS table) and every consumer lane adds
// its five canonical words into sums[k][word]: a 16-byte load, a mod-p add and
// a 16-byte store per field -- the decoded words never reach HBM.  The sums
// are read again by the next party's launch, so the loads and stores are plain
// (no nontemporal hint).  Launches of one session run in order on one stream:
// the read-modify-write is not atomic.
//
// Bad characters: the decode reports its party-local value (field * nchars +
// offset) into a workgroup word in LDS; one lane then min-combines the whole
// call's encoding, (5 party + field) * nchars + offset, into the session's
// verdict word and into the call's own (bad_call, may be null).
//
// SEG (include/amphora_client_batch.h): K objects' texts in the slotted layout
// above, the sums packed on woff.  The workgroup decodes one tile of ONE
// object (seg_tile / seg_fields, the lane-by-lane last tile included) and adds
// into sums[k][woff[o] + word]; bad_session / bad_call are arrays of n_objects
// words and take (5 party + field) * nchars_o + offset at [o].  The shape of
// the launch is the kernel's one argument that differs between the forms, so
// the one-secret form keeps its arguments and its code.
//
// BODY (with SEG; include/amphora_client_bodies.h): the K objects' texts lie
// where the party's response bodies hold them.  All five text pointers are ONE
// 16-byte aligned buffer (tx.t[0][0]) and object o's field k starts at byte
// starts[k][o] of it, any residue mod 16 -- five scalar loads beside seg_tile's.
// Fast lanes fetch through text_unit<true> (aligned granules, funnelled), the
// last tile's per-character lanes read byte by byte as ever.  An object whose
// first start is kBodyAbsent is a workgroup-uniform early exit: it reports
// (5 party) * nchars_o -- what a slot of NUL bytes reports in the slotted form
// -- and adds nothing to the sums.  Everything else is the SEG form's.
constexpr uint64_t kBodyAbsent = ~(uint64_t)0;  // AMPH_BODY_ABSENT
template <bool SEG, bool BODY = false>
struct AccShape {  // one secret: its words, its text's characters and '=' padding
  size_t words, nchars;
  uint32_t pad;
};
template <>
struct AccShape<true> {  // the slotted layout's device tables
  const uint64_t *woff, *toff;
  size_t n_objects;
};
template <>
struct AccShape<true, true> {  // the word table and starts[5][n_objects]
  const uint64_t *woff, *starts;
  size_t n_objects;
};

template <bool BIG, int BS, bool SEG, bool BODY = false>
__global__ __launch_bounds__(BS) AMPH_WIRE_OCC void k_acc_b64(TextSet tx, int party, AccShape<SEG, BODY> sh, SumSet sums,
                                            unsigned long long* bad_session, unsigned long long* bad_call, Fp f) {
  static_assert(SEG || !BODY, "the any-alignment form is a form of the K-secret kernel");
  __shared__ uint32_t lds[WireGroups<1>::bufs < 2 ? 2 : WireGroups<1>::bufs][3 * BS];
  __shared__ uint32_t lutw[kLutBytes / 4];
  __shared__ unsigned long long wg_bad;
  uint8_t* lutp = reinterpret_cast<uint8_t*>(lutw);
  if constexpr (SEG && BODY) {
    SegTile s;
    // (field 0's starts stand where the slotted form's text offsets do: s.toff is starts[0][o])
    const bool real = seg_tile<BS>(sh.woff, sh.starts, sh.n_objects, s);
    uint64_t st[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 1; k < 5; ++k) st[k] = sh.starts[k * sh.n_objects + s.o];  // s.o < n_objects whatever the table holds
    b64_lut_fill(lutp);
    if (threadIdx.x == 0) wg_bad = ~0ULL;
    __syncthreads();
    if (!real) return;  // (the whole workgroup)
    st[0] = s.toff;
    if (st[0] == kBodyAbsent) {  // (the whole workgroup)
      if (threadIdx.x == 0) {
        const unsigned long long v = (unsigned long long)(5 * (size_t)party) * s.nchars;
        atomicMin(bad_session + s.o, v);
        if (bad_call) atomicMin(bad_call + s.o, v);
      }
      return;
    }
    TextSet bt;
#pragma unroll
    for (int k = 0; k < 5; ++k) bt.t[k][0] = tx.t[0][0] + st[k];
    s.toff = 0;
    W4 acc[5];
    uint4 raw[5][1];
    seg_fields<1, BIG, BS, true>(bt, 1, s, raw, lds, acc, &wg_bad, f, lutp);
    const size_t word = s.tile * Wire<BS>::words + threadIdx.x;
    if (threadIdx.x < Wire<BS>::words && word < s.words) {  // s.w0 + s.words <= T: seg_tile's clamp
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        uint4* p = sums.s[k] + s.w0 + word;
        *p = u4(mod_add(w4(*p), acc[k], f));
      }
    }
    __syncthreads();  // every lane's report is in wg_bad
    if (threadIdx.x == 0 && wg_bad != ~0ULL) {
      const unsigned long long v = wg_bad + (unsigned long long)(5 * (size_t)party) * s.nchars;
      atomicMin(bad_session + s.o, v);
      if (bad_call) atomicMin(bad_call + s.o, v);
    }
  } else if constexpr (SEG) {
    SegTile s;
    const bool real = seg_tile<BS>(sh.woff, sh.toff, sh.n_objects, s);  // its table loads fly during the fill
    b64_lut_fill(lutp);
    if (threadIdx.x == 0) wg_bad = ~0ULL;
    __syncthreads();
    if (!real) return;  // (the whole workgroup)
    W4 acc[5];
    uint4 raw[5][1];
    seg_fields<1, BIG, BS>(tx, 1, s, raw, lds, acc, &wg_bad, f, lutp);
    const size_t word = s.tile * Wire<BS>::words + threadIdx.x;
    if (threadIdx.x < Wire<BS>::words && word < s.words) {  // s.w0 + s.words <= T: seg_tile's clamp
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        uint4* p = sums.s[k] + s.w0 + word;
        *p = u4(mod_add(w4(*p), acc[k], f));
      }
    }
    __syncthreads();  // every lane's report is in wg_bad
    if (threadIdx.x == 0 && wg_bad != ~0ULL) {
      const unsigned long long v = wg_bad + (unsigned long long)(5 * (size_t)party) * s.nchars;
      atomicMin(bad_session + s.o, v);
      if (bad_call) atomicMin(bad_call + s.o, v);
    }
  } else {
    const size_t words = sh.words, nchars = sh.nchars;
    const uint32_t pad = sh.pad;
    b64_lut_fill(lutp);
    if (threadIdx.x == 0) wg_bad = ~0ULL;
    __syncthreads();
    W4 acc[5];
    uint4 raw[5][1];
    const bool fast = ((size_t)blockIdx.x + 1) * Wire<BS>::chars + 4 <= nchars;
    if (fast) {
      wire_load<1, BS>(tx, raw, blockIdx.x);
      wire_fields<1, BIG, true, BS>(tx, 1, nchars, pad, words, raw, lds, acc, &wg_bad, f, blockIdx.x, lutp);
    } else {
      wire_fields<1, BIG, false, BS>(tx, 1, nchars, pad, words, raw, lds, acc, &wg_bad, f, blockIdx.x, lutp);
    }
    const size_t word = (size_t)blockIdx.x * Wire<BS>::words + threadIdx.x;
    if (threadIdx.x < Wire<BS>::words && word < words) {
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        uint4* p = sums.s[k] + word;
        *p = u4(mod_add(w4(*p), acc[k], f));
      }
    }
    __syncthreads();  // every lane's report is in wg_bad
    if (threadIdx.x == 0 && wg_bad != ~0ULL) {
      const unsigned long long v = wg_bad + (unsigned long long)(5 * (size_t)party) * nchars;
      atomicMin(bad_session, v);
      if (bad_call) atomicMin(bad_call, v);
    }
  }
}

// K_MASK from the sums: k_mask_b64 / k_mask_json with acc[5] loaded from the
// session's sums instead of decoded -- mask_tile_out unchanged, so the tile
// ownership of the 24-character records and the 37-byte framed records is
// the whole call's.
template <int BS, bool JSON>
__global__ __launch_bounds__(BS) void k_mask_sums(SumSet sums, size_t words, const uint4* secrets, size_t n_secrets,
                                                  uint4* out16, char* out24, unsigned long long* ff, Fp f) {
  constexpr int WW = Wire<BS>::words;
  // (the framed text image of WW records: 37 WW + 4 bytes, as k_mask_json)
  __shared__ __attribute__((aligned(16))) uint32_t lds[JSON ? 3 : 1][3 * BS];
  static_assert(3 * 3 * BS * 4 >= kJsonRec * WW + 4, "the text image fits the buffers");
  W4 acc[5];
  const size_t word = (size_t)blockIdx.x * WW + threadIdx.x;
  const bool in = threadIdx.x < WW && word < words;
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = w4(in ? sums.s[k][word] : make_uint4(0, 0, 0, 0));
  uint4 s = make_uint4(0, 0, 0, 0);
  if (threadIdx.x < WW && word < n_secrets) s = ld(secrets + word);
  mask_tile_out<1, BS, JSON>(blockIdx.x, words, s, n_secrets, acc, out16, out24, ff, lds, f);
}

// k_mask_sums for K objects (include/amphora_client_batch.h): the sums, the
// secrets and out16 / out24 packed on woff, one secret per mask word, ff an
// array of n_objects words with object-local indices.  The workgroup's object
// and tile come from the word table alone (wire_tile_find; the word range
// clamped into [0, woff[n_objects]] as seg_tile does), and mask_tile_out runs
// unchanged with the object's own tile index and word count.  JSON: object
// o's framed text goes to out24 + ooff[o] (a multiple of 16), the "[]" of an
// object of no words comes from workgroup g(o) as in k_mask_json_seg.
template <int BS, bool JSON>
__global__ __launch_bounds__(BS) void k_mask_sums_seg(SumSet sums, const uint64_t* woff, const uint64_t* ooff,
                                                      size_t n_objects, const uint4* secrets, uint4* out16,
                                                      char* out24, unsigned long long* ff, Fp f) {
  constexpr int WW = Wire<BS>::words;
  static_assert(WW == kWireTileWords, "wiretiles.hpp's tile is this workgroup's");
  // (the framed text image of WW records: 37 WW + 4 bytes, as k_mask_json)
  __shared__ __attribute__((aligned(16))) uint32_t lds[JSON ? 3 : 1][3 * BS];
  static_assert(3 * 3 * BS * 4 >= kJsonRec * WW + 4, "the text image fits the buffers");
  const WireTile wt = wire_tile_find(woff, n_objects, blockIdx.x, WW);
  const uint64_t T = woff[n_objects];
  const uint64_t a = woff[wt.object], b = woff[wt.object + 1];
  const uint64_t w0 = a < T ? a : T, w1 = b < w0 ? w0 : (b < T ? b : T);
  const size_t words = (size_t)(w1 - w0);
  if (!wire_tile_real(wt.local, words, WW)) {  // (the whole workgroup)
    if constexpr (JSON) {
      char* dst = out24 + ooff[wt.object];
      if (words == 0 && wt.local == 0 && threadIdx.x < 2) dst[threadIdx.x] = threadIdx.x ? ']' : '[';
    }
    return;
  }
  W4 acc[5];
  const size_t word = wt.local * WW + threadIdx.x;
  const bool in = threadIdx.x < WW && word < words;
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = w4(in ? sums.s[k][w0 + word] : make_uint4(0, 0, 0, 0));
  uint4 s = make_uint4(0, 0, 0, 0);
  if (in) s = ld(secrets + w0 + word);
  if constexpr (JSON)
    mask_tile_out<1, BS, true>(wt.local, words, s, words, acc, nullptr, out24 + ooff[wt.object], ff + wt.object, lds,
                               f);
  else
    mask_tile_out<1, BS>(wt.local, words, s, words, acc, out16 ? out16 + w0 : nullptr,
                         out24 ? out24 + 24 * w0 : nullptr, ff + wt.object, lds, f);
}

}  // namespace

#ifndef AMPH_WIRE_KERNELS_ONLY  // (tools/ubench: the kernels without the launchers' instantiations)
hipError_t launch_rv_b64(const TextSet& tx, int n, size_t words, size_t nchars, uint32_t pad,
                         uint4* out_y, unsigned long long* ff, unsigned long long* bad, const Fp& f,
                         const LaunchCfg& c) {
  if (words == 0) return hipSuccess;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)((words + Wire<BS>::words - 1) / Wire<BS>::words));
#define L(NP, BIG) AMPH_LAUNCH((k_rv_b64<NP, BIG, BS>), g, dim3(BS), c, tx, n, words, nchars, pad, out_y, ff, bad, f)
  if (f.big) { AMPH_DISPATCH_NP(n, true, L) } else { AMPH_DISPATCH_NP_SMALL2(n, L) }
#undef L
  return hipGetLastError();
}

hipError_t launch_mask_b64(const TextSet& tx, int n, size_t words, size_t nchars, uint32_t pad,
                           const uint4* secrets, size_t n_secrets, uint4* out16, char* out24,
                           unsigned long long* ff, unsigned long long* bad, const Fp& f,
                           const LaunchCfg& c) {
  if (words == 0) return hipSuccess;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)((words + Wire<BS>::words - 1) / Wire<BS>::words));
#define L(NP, BIG) AMPH_LAUNCH((k_mask_b64<NP, BIG, BS>), g, dim3(BS), c, tx, n, words, nchars, pad, secrets, n_secrets, out16, out24, ff, bad, f)
  if (f.big) { AMPH_DISPATCH_NP(n, true, L) } else { AMPH_DISPATCH_NP_SMALL2(n, L) }
#undef L
  return hipGetLastError();
}

hipError_t launch_mask_json(const TextSet& tx, int n, size_t words, size_t nchars, uint32_t pad,
                            const uint4* secrets, size_t n_secrets, char* out_text,
                            unsigned long long* ff, unsigned long long* bad, const Fp& f,
                            const LaunchCfg& c) {
  if (words == 0) return hipSuccess;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)((words + Wire<BS>::words - 1) / Wire<BS>::words));
#define L(NP, BIG) AMPH_LAUNCH((k_mask_json<NP, BIG, BS>), g, dim3(BS), c, tx, n, words, nchars, pad, secrets, n_secrets, out_text, ff, bad, f)
  if (f.big) { AMPH_DISPATCH_NP(n, true, L) } else { AMPH_DISPATCH_NP_SMALL2(n, L) }
#undef L
  return hipGetLastError();
}

hipError_t launch_rv_b64_seg(const TextSet& tx, int n, const uint64_t* woff, const uint64_t* toff,
                             size_t n_objects, size_t grid, uint4* out_y, unsigned long long* ff,
                             unsigned long long* bad, const Fp& f, const LaunchCfg& c) {
  if (grid == 0 || n_objects == 0) return hipSuccess;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)grid);
#define L(NP, BIG) AMPH_LAUNCH((k_rv_b64_seg<NP, BIG, BS>), g, dim3(BS), c, tx, n, woff, toff, n_objects, out_y, ff, bad, f)
  if (f.big) { AMPH_DISPATCH_NP(n, true, L) } else { AMPH_DISPATCH_NP_SMALL2(n, L) }
#undef L
  return hipGetLastError();
}

hipError_t launch_mask_b64_seg(const TextSet& tx, int n, const uint64_t* woff, const uint64_t* toff,
                               size_t n_objects, size_t grid, const uint4* secrets, uint4* out16, char* out24,
                               unsigned long long* ff, unsigned long long* bad, const Fp& f,
                               const LaunchCfg& c) {
  if (grid == 0 || n_objects == 0) return hipSuccess;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)grid);
#define L(NP, BIG) AMPH_LAUNCH((k_mask_b64_seg<NP, BIG, BS>), g, dim3(BS), c, tx, n, woff, toff, n_objects, secrets, out16, out24, ff, bad, f)
  if (f.big) { AMPH_DISPATCH_NP(n, true, L) } else { AMPH_DISPATCH_NP_SMALL2(n, L) }
#undef L
  return hipGetLastError();
}

hipError_t launch_mask_json_seg(const TextSet& tx, int n, const uint64_t* woff, const uint64_t* toff,
                                const uint64_t* ooff, size_t n_objects, size_t grid, const uint4* secrets,
                                char* out_text, unsigned long long* ff, unsigned long long* bad, const Fp& f,
                                const LaunchCfg& c) {
  if (grid == 0 || n_objects == 0) return hipSuccess;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)grid);
#define L(NP, BIG) AMPH_LAUNCH((k_mask_json_seg<NP, BIG, BS>), g, dim3(BS), c, tx, n, woff, toff, ooff, n_objects, secrets, out_text, ff, bad, f)
  if (f.big) { AMPH_DISPATCH_NP(n, true, L) } else { AMPH_DISPATCH_NP_SMALL2(n, L) }
#undef L
  return hipGetLastError();
}

hipError_t launch_acc_b64(const TextSet& tx, int party, size_t words, size_t nchars, uint32_t pad,
                          const SumSet& sums, unsigned long long* bad_session, unsigned long long* bad_call,
                          const Fp& f, const LaunchCfg& c) {
  if (words == 0) return hipSuccess;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)((words + Wire<BS>::words - 1) / Wire<BS>::words));
  const AccShape<false> sh{words, nchars, pad};
  if (f.big)
    AMPH_LAUNCH((k_acc_b64<true, BS, false>), g, dim3(BS), c, tx, party, sh, sums, bad_session, bad_call, f);
  else
    AMPH_LAUNCH((k_acc_b64<false, BS, false>), g, dim3(BS), c, tx, party, sh, sums, bad_session, bad_call, f);
  return hipGetLastError();
}

hipError_t launch_acc_b64_seg(const TextSet& tx, int party, const uint64_t* woff, const uint64_t* toff,
                              size_t n_objects, size_t grid, const SumSet& sums, unsigned long long* bad_session,
                              unsigned long long* bad_call, const Fp& f, const LaunchCfg& c) {
  if (grid == 0 || n_objects == 0) return hipSuccess;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)grid);
  const AccShape<true> sh{woff, toff, n_objects};
  if (f.big)
    AMPH_LAUNCH((k_acc_b64<true, BS, true>), g, dim3(BS), c, tx, party, sh, sums, bad_session, bad_call, f);
  else
    AMPH_LAUNCH((k_acc_b64<false, BS, true>), g, dim3(BS), c, tx, party, sh, sums, bad_session, bad_call, f);
  return hipGetLastError();
}

hipError_t launch_acc_b64_bodies(const char* buffer, int party, const uint64_t* woff, const uint64_t* starts,
                                 size_t n_objects, size_t grid, const SumSet& sums, unsigned long long* bad_session,
                                 unsigned long long* bad_call, const Fp& f, const LaunchCfg& c) {
  if (grid == 0 || n_objects == 0) return hipSuccess;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)grid);
  TextSet tx{};
  tx.t[0][0] = buffer;
  const AccShape<true, true> sh{woff, starts, n_objects};
  if (f.big)
    AMPH_LAUNCH((k_acc_b64<true, BS, true, true>), g, dim3(BS), c, tx, party, sh, sums, bad_session, bad_call, f);
  else
    AMPH_LAUNCH((k_acc_b64<false, BS, true, true>), g, dim3(BS), c, tx, party, sh, sums, bad_session, bad_call, f);
  return hipGetLastError();
}

hipError_t launch_mask_sums_seg(const SumSet& sums, const uint64_t* woff, const uint64_t* ooff, size_t n_objects,
                                size_t grid, const uint4* secrets, uint4* out16, char* out24, char* out_text,
                                unsigned long long* ff, const Fp& f, const LaunchCfg& c) {
  if (grid == 0 || n_objects == 0) return hipSuccess;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)grid);
  if (out_text)
    AMPH_LAUNCH((k_mask_sums_seg<BS, true>), g, dim3(BS), c, sums, woff, ooff, n_objects, secrets, nullptr, out_text,
                ff, f);
  else
    AMPH_LAUNCH((k_mask_sums_seg<BS, false>), g, dim3(BS), c, sums, woff, ooff, n_objects, secrets, out16, out24, ff,
                f);
  return hipGetLastError();
}

hipError_t launch_mask_sums(const SumSet& sums, size_t words, const uint4* secrets, size_t n_secrets, uint4* out16,
                            char* out24, char* out_text, unsigned long long* ff, const Fp& f, const LaunchCfg& c) {
  if (words == 0) return hipSuccess;
  constexpr int BS = kWireBlock;
  const dim3 g((unsigned)((words + Wire<BS>::words - 1) / Wire<BS>::words));
  if (out_text)
    AMPH_LAUNCH((k_mask_sums<BS, true>), g, dim3(BS), c, sums, words, secrets, n_secrets, nullptr, out_text, ff, f);
  else
    AMPH_LAUNCH((k_mask_sums<BS, false>), g, dim3(BS), c, sums, words, secrets, n_secrets, out16, out24, ff, f);
  return hipGetLastError();
}

#endif  // AMPH_WIRE_KERNELS_ONLY

}  // namespace amph
