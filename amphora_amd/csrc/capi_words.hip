// C ABI of libamphora_hip (declared in include/amphora.h): the per-word entry
// points -- each one launch, written once for both modes (run_words,
// capi_internal.hpp) -- the ragged last word of recombineObject's party
// arrays, the packed and gathered many-secret calls, the synthetic data
// generators and the stream probe.
#include "capi_internal.hpp"
#include "seglookup.hpp"

namespace {
// recombineObject's word count and ragged party arrays (client
// SecretShareUtil.java:75,87-88): W = party 0's length / 16, and party j's
// word i is Arrays.copyOfRange(share_j, 16 i, 16 i + 16) -- a longer array
// is cut, a word running past the end of a shorter one is zero-padded, and a
// word STARTING past the end (16 i > length) throws
// ArrayIndexOutOfBoundsException (AMPH_E_RANGE).  So only word W-1 can be
// padded: *ragged says some party ends inside it (16 (W-1) <= length < 16 W).
// Callers that cannot take a padded word pass ragged = nullptr and get
// AMPH_E_LEN for it.
int party_words(const size_t* lens, int n, size_t* words, bool* ragged) {
  const size_t w = lens[0] / AMPH_WORD_WIDTH;
  bool rg = false;
  for (int j = 1; j < n; ++j) {
    if (lens[j] >= AMPH_WORD_WIDTH * w) continue;
    if (lens[j] + AMPH_WORD_WIDTH < AMPH_WORD_WIDTH * w)
      return fail(AMPH_E_RANGE, "Arrays.copyOfRange: word " +
                                    std::to_string(lens[j] / AMPH_WORD_WIDTH + 1) +
                                    " starts past the end of party " + std::to_string(j) + "'s " +
                                    std::to_string(lens[j]) + "-byte share array (" +
                                    std::to_string(w) + " words from party 0)");
    rg = true;
  }
  if (rg && !ragged) return fail(AMPH_E_LEN, "The provided shares must be of the same length");
  if (ragged) *ragged = rg;
  *words = w;
  return AMPH_OK;
}

int odo_words(const amph_odo* odos, int n, size_t* words, bool* ragged = nullptr) {
  if (!odos || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with a non-null ODO array");
  size_t lens[AMPH_MAX_PARTIES];
  for (int j = 0; j < n; ++j) lens[j] = odos[j].nbytes;
  if (int st = party_words(lens, n, words, ragged)) return st;
  for (int j = 0; j < n; ++j)
    if (*words && odos[j].nbytes && (!odos[j].secret_shares || !odos[j].r_shares || !odos[j].v_shares ||
                   !odos[j].w_shares || !odos[j].u_shares))
      return fail(AMPH_E_PARAM, "null ODO field");
  return AMPH_OK;
}

const uint8_t* odo_field(const amph_odo& o, int k) {
  switch (k) {
    case 0: return o.secret_shares;
    case 1: return o.r_shares;
    case 2: return o.v_shares;
    case 3: return o.w_shares;
    default: return o.u_shares;
  }
}

int check_dev_odos(const amph_odo* odos, int n) {
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < 5; ++k)
      if (int st = check_dev_words({odo_field(odos[j], k)})) return st;
  return AMPH_OK;
}

// The five fields of n parties as word arrays, field-major (array k * n + j is
// field k of party j), starting at word `base`; odo_set reads device pointers
// in the same layout.
WordArrays odo_arrays(const amph_odo* odos, int n, size_t base = 0) {
  WordArrays a;
  for (int k = 0; k < 5; ++k)
    for (int j = 0; j < n; ++j) a.push_back(arr_in(odo_field(odos[j], k), 16, 16, base));
  return a;
}
amph::OdoSet odo_set(const uint4* const* f, int n) {
  amph::OdoSet set{};
  for (int k = 0; k < 5; ++k)
    for (int j = 0; j < n; ++j) set.f[k][j] = f[k * n + j];
  return set;
}
amph::OdoSet odo_set(const amph_odo* odos, int n) {  // device-mode ODOs
  const uint4* f[5 * AMPH_MAX_PARTIES];
  for (int k = 0; k < 5; ++k)
    for (int j = 0; j < n; ++j) f[k * n + j] = (const uint4*)odo_field(odos[j], k);
  return odo_set(f, n);
}

// n parties' signed diffs (64-byte magnitude pairs, then the 4-byte sign
// words) as word arrays, and the kernels' SignedSet over their device pointers
WordArrays diff_arrays(const uint8_t* const* mags, const uint8_t* const* negs, int n) {
  WordArrays a;
  for (int j = 0; j < n; ++j) a.push_back(arr_in(mags[j], 64));
  for (int j = 0; j < n; ++j) a.push_back(arr_in(negs[j], 4, 0));
  return a;
}
amph::SignedSet diff_set(const DevIn& din, int n) {
  amph::SignedSet set{};
  for (int j = 0; j < n; ++j) {
    set.mag[j] = din[j];
    set.neg[j] = (const uint32_t*)din[n + j];
  }
  return set;
}

// ---- the ragged last word (party_words) --------------------------------------
// A ragged call runs words [0, W-1) as usual (every party holds them in full)
// and word W-1 as a one-word call over zero-padded copies of each array's
// bytes [16 (W-1), length): what Arrays.copyOfRange hands fromGfp.

// Stage array i's bytes [off, min(len[i], off + 16)), zero-padded, into the
// 16-byte word dst + 16 i.  src: host pointers (flags 0), amph_host_array
// descriptors (AMPH_F_HOST_IO; read through their callback) or device
// pointers (AMPH_F_DEVICE: dst is device memory, the copies go on s).
int stage_tail(const uint8_t* const* src, const size_t* len, int m, size_t off, uint8_t* dst,
               uint32_t flags, hipStream_t s) {
  if (flags & AMPH_F_DEVICE) {
    HIP_TRY(hipMemsetAsync(dst, 0, 16 * (size_t)m, s));
    for (int i = 0; i < m; ++i) {
      const size_t nb = std::min<size_t>(16, len[i] - off);
      if (nb) HIP_TRY(hipMemcpyAsync(dst + 16 * i, src[i] + off, nb, hipMemcpyDeviceToDevice, s));
    }
    return AMPH_OK;
  }
  std::memset(dst, 0, 16 * (size_t)m);
  for (int i = 0; i < m; ++i) {
    const size_t nb = std::min<size_t>(16, len[i] - off);
    if (!nb) continue;
    if (flags & AMPH_F_HOST_IO) {
      const amph_host_array* a = (const amph_host_array*)src[i];
      if (a->read(a, off, nb, dst + 16 * i)) return fail(AMPH_E_PARAM, "a host-array read callback failed");
    } else {
      std::memcpy(dst + 16 * i, src[i] + off, nb);
    }
  }
  return AMPH_OK;
}

// one host word to / from an output / input argument (descriptor under AMPH_F_HOST_IO)
int put_word(uint8_t* dst, size_t off, const uint8_t* w, uint32_t flags) {
  if (flags & AMPH_F_HOST_IO) {
    const amph_host_array* a = (const amph_host_array*)dst;
    if (a->write(a, off, 16, w)) return fail(AMPH_E_PARAM, "a host-array write callback failed");
  } else {
    std::memcpy(dst + off, w, 16);
  }
  return AMPH_OK;
}

// Device scratch of one ragged call: the staged words and a verdict word.
struct TailScratch {
  uint8_t* p = nullptr;
  hipStream_t s = nullptr;
  ~TailScratch() {
    if (p) (void)hipFreeAsync(p, s);
  }
};

// The ODO calls over ragged parties: `masked` = false runs
// amph_recombine_verify, true amph_mask_input (n_secrets <= W).
int ragged_odo_call(amph_ctx* c, const amph_odo* odos, int n, size_t W, bool masked, const uint8_t* secrets,
                    size_t n_secrets, uint8_t* out, int64_t* first_fail, uint32_t flags, void* stream) {
  const size_t off = AMPH_WORD_WIDTH * (W - 1);
  const bool dev = flags & AMPH_F_DEVICE, io = flags & AMPH_F_HOST_IO;
  hipStream_t s = (hipStream_t)stream;
  amph_odo head[AMPH_MAX_PARTIES], tail[AMPH_MAX_PARTIES];
  const uint8_t* src[5 * AMPH_MAX_PARTIES];
  size_t len[5 * AMPH_MAX_PARTIES];
  for (int j = 0; j < n; ++j) {
    head[j] = odos[j];
    head[j].nbytes = off;
    for (int k = 0; k < 5; ++k) {
      src[k * n + j] = odo_field(odos[j], k);
      len[k * n + j] = odos[j].nbytes;
    }
  }
  // words [0, W-1): secrets below W-1 masked there, word W-1's secret (if
  // any) in the tail; the rest verify only, as amph_mask_input does
  const size_t hs = std::min(n_secrets, W - 1), ts = n_secrets == W ? 1 : 0;
  int64_t hf = -1;
  int64_t* hff = dev ? first_fail : &hf;
  const int st = masked ? amph_mask_input(c, head, n, secrets, hs, out, hff, flags, stream)
                        : amph_recombine_verify(c, head, n, out, hff, flags, stream);
  if (st != AMPH_OK && st != AMPH_E_VERIFY) return st;
  auto point = [&](uint8_t* base) {
    for (int j = 0; j < n; ++j) {
      tail[j] = amph_odo{base + 16 * (0 * n + j), base + 16 * (1 * n + j), base + 16 * (2 * n + j),
                         base + 16 * (3 * n + j), base + 16 * (4 * n + j), 16};
    }
  };
  if (dev) {
    HIP_TRY(use_device(c->device));
    TailScratch sc;
    sc.s = s;
    HIP_TRY(hipMallocAsync((void**)&sc.p, 16 * 5 * (size_t)n + 16, s));
    int64_t* tf = (int64_t*)(sc.p + 16 * 5 * n);
    if (int r = stage_tail(src, len, 5 * n, off, sc.p, flags, s)) return r;
    HIP_TRY(hipMemsetAsync(tf, 0x7F, sizeof(int64_t), s));
    point(sc.p);
    const uint32_t tfl = AMPH_F_DEVICE | AMPH_F_ACCUMULATE;
    const int t = masked ? amph_mask_input(c, tail, n, ts ? secrets + off : nullptr, ts,
                                           ts ? out + off : nullptr, tf, tfl, stream)
                         : amph_recombine_verify(c, tail, n, out + off, tf, tfl, stream);
    if (t != AMPH_OK) return t;
    hipError_t e = amph::launch_ff_merge((unsigned long long*)first_fail, (const unsigned long long*)tf, W - 1, s);
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_ff_merge");
  }
  uint8_t words[16 * 5 * AMPH_MAX_PARTIES], sec[16], res[16];
  if (int r = stage_tail(src, len, 5 * n, off, words, flags, nullptr)) return r;
  point(words);
  if (ts) {
    if (io) {
      const amph_host_array* a = (const amph_host_array*)secrets;
      if (a->read(a, off, 16, sec)) return fail(AMPH_E_PARAM, "a host-array read callback failed");
    } else {
      std::memcpy(sec, secrets + off, 16);
    }
  }
  int64_t tf = -1;
  const int t = masked ? amph_mask_input(c, tail, n, ts ? sec : nullptr, ts, ts ? res : nullptr, &tf, 0, nullptr)
                       : amph_recombine_verify(c, tail, n, res, &tf, 0, nullptr);
  if (t != AMPH_OK && t != AMPH_E_VERIFY) return t;
  if ((!masked || ts) && put_word(out, off, res, flags)) return AMPH_E_PARAM;
  const int64_t v = st == AMPH_E_VERIFY ? hf : (t == AMPH_E_VERIFY ? (int64_t)(W - 1) : -1);
  if (first_fail) *first_fail = v;
  return v >= 0 ? AMPH_E_VERIFY : AMPH_OK;
}

// ---- packed and gathered calls (amph_*_packed, amph_*_batch) --------------------
// Packed parties have no ragged form: every party holds all T words.
int packed_words(const amph_odo* odos, int n, size_t* words) {
  if (!odos || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with a non-null ODO array");
  for (int j = 0; j < n; ++j)
    if (odos[j].nbytes != odos[0].nbytes || odos[j].nbytes % AMPH_WORD_WIDTH)
      return fail(AMPH_E_LEN, "packed ODOs: party " + std::to_string(j) + " holds " +
                                  std::to_string(odos[j].nbytes) + " bytes, party 0 " +
                                  std::to_string(odos[0].nbytes) + " (equal multiples of 16 required)");
  *words = odos[0].nbytes / AMPH_WORD_WIDTH;
  for (int j = 0; j < n; ++j)
    if (*words && (!odos[j].secret_shares || !odos[j].r_shares || !odos[j].v_shares || !odos[j].w_shares ||
                   !odos[j].u_shares))
      return fail(AMPH_E_PARAM, "null ODO field");
  return AMPH_OK;
}

// a host offsets table: offsets[0] = 0, nondecreasing, offsets[n_objects] = words
int check_offsets(const uint64_t* offsets, size_t n_objects, size_t words) {
  if (!offsets) return fail(AMPH_E_PARAM, "null offsets table");
  if (offsets[0] != 0) return fail(AMPH_E_PARAM, "offsets[0] must be 0");
  for (size_t o = 0; o < n_objects; ++o)
    if (offsets[o + 1] < offsets[o])
      return fail(AMPH_E_PARAM, "offsets must not decrease (entry " + std::to_string(o + 1) + ")");
  if (offsets[n_objects] != words)
    return fail(AMPH_E_PARAM, "offsets[n_objects] = " + std::to_string(offsets[n_objects]) +
                                  " must equal the ODO word count " + std::to_string(words));
  return AMPH_OK;
}

// Both packed calls: `masked` = false runs K_RV, true K_MASK (secrets != null).
int packed_call(amph_ctx* c, const amph_odo* odos, int n, const uint64_t* offsets, size_t n_objects, bool masked,
                const uint8_t* secrets, uint8_t* out, int64_t* first_fail, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (n_objects == 0) return AMPH_OK;
  size_t T;
  if (int st = packed_words(odos, n, &T)) return st;
  if (!offsets || !first_fail) return fail(AMPH_E_PARAM, "null offsets table or first_fail array");
  if (T && (!out || (masked && !secrets))) return fail(AMPH_E_PARAM, masked ? "null secrets/output" : "null output");
  c = first_device(c);  // a multi-device context runs packed calls on its first device
  const auto launch = [&](const DevIn& din, const DevOut& dout, size_t cnt, size_t base, const uint64_t* tab,
                          unsigned long long* ff, const amph::LaunchCfg& lc) {
    const amph::OdoSet set = odo_set(din.data(), n);
    return masked ? amph::launch_mask_input_seg(set, n, cnt, din[5 * n], dout[0], ff, tab, n_objects, base, c->f, lc)
                  : amph::launch_recombine_verify_seg(set, n, cnt, dout[0], ff, tab, n_objects, base, c->f, lc);
  };
  if (flags & AMPH_F_DEVICE) {
    if (int st = check_dev_odos(odos, n)) return st;
    if (int st = check_dev_words({secrets, out})) return st;
    if (((uintptr_t)offsets | (uintptr_t)first_fail) & 7)
      return fail(AMPH_E_PARAM, "device offsets and first_fail arrays must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(use_device(c->device));
    if (!(flags & AMPH_F_ACCUMULATE)) HIP_TRY(hipMemsetAsync(first_fail, 0x7F, 8 * n_objects, s));
    DevIn din;
    for (int k = 0; k < 5; ++k)
      for (int j = 0; j < n; ++j) din.push_back((const uint4*)odo_field(odos[j], k));
    if (masked) din.push_back((const uint4*)secrets);
    const hipError_t e = launch(din, DevOut{(uint4*)out}, T, 0, offsets, (unsigned long long*)first_fail,
                                cfg(c, s, T));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, masked ? "k_mask_seg" : "k_rv_seg");
  }
  if (int st = check_offsets(offsets, n_objects, T)) return st;
  WordArrays ins = odo_arrays(odos, n);
  if (masked) ins.push_back(arr_in(secrets, 16));
  std::lock_guard<std::mutex> g(c->mu);
  return run_packed(c, T, ins, {arr_out(out, 16)}, offsets, n_objects, first_fail, launch);
}

// One packed array of a gathered call as an amph_host_array: its read / write
// walk the objects' separate pieces (piece[o] holds object o's words), so the
// pipeline's staging copies gather and scatter in the same pass that moves
// the bytes into page-locked memory.
struct Gather {
  amph_host_array a{};
  std::vector<uint8_t*> piece;
  const uint64_t* offsets = nullptr;
  size_t n_objects = 0;
};
int gather_rw(const amph_host_array* a, size_t off, size_t bytes, uint8_t* buf, bool write) {
  const Gather* g = (const Gather*)a->user;
  size_t o = amph::seg_find(g->offsets, g->n_objects, off / AMPH_WORD_WIDTH);
  while (bytes) {
    const size_t lo = AMPH_WORD_WIDTH * g->offsets[o], hi = AMPH_WORD_WIDTH * g->offsets[o + 1];
    if (off >= hi) {  // an empty object, or this one is done
      ++o;
      continue;
    }
    const size_t nb = std::min(bytes, hi - off);
    if (write) std::memcpy(g->piece[o] + (off - lo), buf, nb);
    else std::memcpy(buf, g->piece[o] + (off - lo), nb);
    buf += nb, off += nb, bytes -= nb;
  }
  return 0;
}
void gather_init(Gather& g, const std::vector<uint64_t>& offsets) {
  g.offsets = offsets.data();
  g.n_objects = offsets.size() - 1;
  g.piece.resize(g.n_objects);
  g.a.user = &g;
  g.a.read = [](const amph_host_array* a, size_t off, size_t bytes, void* dst) {
    return gather_rw(a, off, bytes, (uint8_t*)dst, false);
  };
  g.a.write = [](const amph_host_array* a, size_t off, size_t bytes, const void* src) {
    return gather_rw(a, off, bytes, (uint8_t*)const_cast<void*>(src), true);
  };
}
WordArray gather_array(const Gather& g, bool out) { return WordArray{nullptr, 16, 16, out, 0, &g.a}; }

// Both gathered calls: odos[o * n + j] is party j's ODO of object o.
int batch_call(amph_ctx* c, const amph_odo* odos, int n, size_t n_objects, bool masked,
               const uint8_t* const* secrets, const size_t* n_secrets, uint8_t* const* out, int64_t* first_fail,
               uint32_t flags) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, "the gathered batch calls take host memory only (flags must be 0)");
  if (n_objects == 0) return AMPH_OK;
  if (!odos || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with a non-null ODO array");
  if (!out || !first_fail || (masked && (!secrets || !n_secrets)))
    return fail(AMPH_E_PARAM, "null pointer array or first_fail array");
  std::vector<uint64_t> offsets(n_objects + 1, 0);
  for (size_t o = 0; o < n_objects; ++o) {
    const amph_odo* po = odos + o * (size_t)n;
    for (int j = 1; j < n; ++j)
      if (po[j].nbytes != po[0].nbytes)
        return fail(AMPH_E_LEN, "object " + std::to_string(o) + ": The provided shares must be of the same length");
    const size_t w = po[0].nbytes / AMPH_WORD_WIDTH;
    if (masked && n_secrets[o] != w)
      return fail(AMPH_E_LEN, "object " + std::to_string(o) + ": " + std::to_string(n_secrets[o]) +
                                  " secret words for " + std::to_string(w) + " input masks");
    for (int j = 0; j < n; ++j)
      if (w && (!po[j].secret_shares || !po[j].r_shares || !po[j].v_shares || !po[j].w_shares || !po[j].u_shares))
        return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null ODO field");
    if (w && (!out[o] || (masked && !secrets[o])))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null secrets/output");
    offsets[o + 1] = offsets[o] + w;
  }
  const size_t T = offsets[n_objects];
  std::vector<Gather> arrays(5 * (size_t)n + (masked ? 2 : 1));
  for (Gather& g : arrays) gather_init(g, offsets);
  for (size_t o = 0; o < n_objects; ++o) {
    for (int k = 0; k < 5; ++k)
      for (int j = 0; j < n; ++j)
        arrays[k * n + j].piece[o] = const_cast<uint8_t*>(odo_field(odos[o * (size_t)n + j], k));
    if (masked) arrays[5 * n].piece[o] = const_cast<uint8_t*>(secrets[o]);
    arrays.back().piece[o] = out[o];
  }
  WordArrays ins;
  for (size_t k = 0; k + 1 < arrays.size(); ++k) ins.push_back(gather_array(arrays[k], false));
  c = first_device(c);
  std::lock_guard<std::mutex> g(c->mu);
  return run_packed(c, T, ins, {gather_array(arrays.back(), true)}, offsets.data(), n_objects, first_fail,
                    [&](const DevIn& din, const DevOut& dout, size_t cnt, size_t base, const uint64_t* tab,
                        unsigned long long* ff, const amph::LaunchCfg& lc) {
                      const amph::OdoSet set = odo_set(din.data(), n);
                      return masked ? amph::launch_mask_input_seg(set, n, cnt, din[5 * n], dout[0], ff, tab,
                                                                  n_objects, base, c->f, lc)
                                    : amph::launch_recombine_verify_seg(set, n, cnt, dout[0], ff, tab, n_objects,
                                                                        base, c->f, lc);
                    });
}

}  // namespace

extern "C" {

int amph_recombine_verify_packed(amph_ctx* c, const amph_odo* odos, int n, const uint64_t* offsets,
                                 size_t n_objects, uint8_t* out_secrets, int64_t* first_fail, uint32_t flags,
                                 void* stream) {
  return packed_call(c, odos, n, offsets, n_objects, false, nullptr, out_secrets, first_fail, flags, stream);
}

int amph_mask_input_packed(amph_ctx* c, const amph_odo* odos, int n, const uint64_t* offsets, size_t n_objects,
                           const uint8_t* secrets, uint8_t* out_masked, int64_t* first_fail, uint32_t flags,
                           void* stream) {
  return packed_call(c, odos, n, offsets, n_objects, true, secrets, out_masked, first_fail, flags, stream);
}

int amph_recombine_verify_batch(amph_ctx* c, const amph_odo* odos, int n, size_t n_objects,
                                uint8_t* const* out_secrets, int64_t* first_fail, uint32_t flags) {
  return batch_call(c, odos, n, n_objects, false, nullptr, nullptr, out_secrets, first_fail, flags);
}

int amph_mask_input_batch(amph_ctx* c, const amph_odo* odos, int n, size_t n_objects,
                          const uint8_t* const* secrets, const size_t* n_secrets, uint8_t* const* out_masked,
                          int64_t* first_fail, uint32_t flags) {
  return batch_call(c, odos, n, n_objects, true, secrets, n_secrets, out_masked, first_fail, flags);
}

int amph_recombine_verify(amph_ctx* c, const amph_odo* odos, int n, uint8_t* out_secrets,
                          int64_t* first_fail, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  size_t W;
  bool ragged;
  if (int st = odo_words(odos, n, &W, &ragged)) return st;
  if (W && !out_secrets) return fail(AMPH_E_PARAM, "null output");
  if (ragged) {
    if (flags & AMPH_F_DEVICE)
      if (int st = check_dev_odos(odos, n)) return st;
    return ragged_odo_call(c, odos, n, W, false, nullptr, 0, out_secrets, first_fail, flags, stream);
  }
  WordArrays arrays = odo_arrays(odos, n);
  arrays.push_back(arr_out(out_secrets, 16));
  return run_words(c, W, arrays, true, first_fail, flags, stream, "k_rv",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long* ff,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_recombine_verify(odo_set(din.data(), n), n, cnt, dout[0], ff, c->f, lc);
                   });
}

int amph_mask_input(amph_ctx* c, const amph_odo* odos, int n, const uint8_t* secrets,
                    size_t n_secrets, uint8_t* out_masked, int64_t* first_fail, uint32_t flags,
                    void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  size_t W;
  bool ragged;
  if (int st = odo_words(odos, n, &W, &ragged)) return st;
  if (n_secrets > W) {
    // The reference verifies every mask before it indexes past the last one
    // (DefaultAmphoraClient.java:153 before :160): a MAC failure outranks the
    // length error.  Verify all W words (n_secrets = 0), then report.  Device
    // mode waits for the verdict here -- an error path, so the stream sync
    // costs nothing a correct call pays.
    int st = amph_mask_input(c, odos, n, nullptr, 0, nullptr, first_fail, flags, stream);
    if (st != AMPH_OK) return st;
    if ((flags & AMPH_F_DEVICE) && first_fail) {
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      int64_t h = 0;
      HIP_TRY(hipMemcpy(&h, first_fail, sizeof h, hipMemcpyDeviceToHost));  // kPageableRule
      if ((uint64_t)h != amph::kNoFail)
        return fail(AMPH_E_VERIFY, "input mask MAC check failed at word " + std::to_string(h));
    }
    return fail(AMPH_E_LEN, "more secret words than verified input masks");
  }
  if (n_secrets && (!secrets || !out_masked)) return fail(AMPH_E_PARAM, "null secrets/output");
  if (ragged) {
    if (flags & AMPH_F_DEVICE)
      if (int st = check_dev_odos(odos, n)) return st;
    return ragged_odo_call(c, odos, n, W, true, secrets, n_secrets, out_masked, first_fail, flags, stream);
  }
  if (flags & AMPH_F_DEVICE) {
    if (int st = check_dev_odos(odos, n)) return st;
    if (int st = check_dev_words({secrets, out_masked})) return st;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(use_device(c->device));
    if (int st = reset_ff_dev(first_fail, flags, s)) return st;
    hipError_t e = amph::launch_mask_input(odo_set(odos, n), n, W, (const uint4*)secrets, n_secrets,
                                           (uint4*)out_masked, (unsigned long long*)first_fail,
                                           c->f, cfg(c, s, W));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_mask");
  }
  // host mode: the masked words, then a verify-only pass over the tail
  // [n_secrets, W) (the Java loop reads inputMasks.get(i) for i < secret.size()
  // only, but verifyOutputDeliveryObjects checked them all): the secrets (one
  // more input) and the output of the first pass are null in the second
  std::lock_guard<std::mutex> g(c->mu);
  auto pass = [&](size_t base, size_t words, bool masked, int64_t* ff_out) {
    WordArrays ins = odo_arrays(odos, n, base), outs;
    if (masked) ins.push_back(arr_in(secrets, 16));
    if (masked) outs.push_back(arr_out(out_masked, 16));
    return run_batched(c, words, ins, outs, true, ff_out,
                       [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long* ff,
                           const amph::LaunchCfg& lc) {
                         return amph::launch_mask_input(odo_set(din.data(), n), n, cnt, masked ? din[5 * n] : nullptr,
                                                        masked ? cnt : 0, masked ? dout[0] : nullptr, ff, c->f, lc);
                       });
  };
  int st = pass(0, n_secrets, true, first_fail);
  if (st != AMPH_OK || n_secrets == W) return st;
  int64_t tf = -1;
  st = pass(n_secrets, W - n_secrets, false, &tf);
  if (st == AMPH_E_VERIFY && first_fail) *first_fail = (int64_t)n_secrets + tf;
  return st;
}

int amph_recombine(amph_ctx* c, const uint8_t* const* shares, int n, size_t nbytes, uint8_t* out,
                   uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (!shares || n < 1 || n > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  const size_t W = nbytes / AMPH_WORD_WIDTH;
  if (W && !out) return fail(AMPH_E_PARAM, "null output");
  for (int j = 0; j < n; ++j)
    if (W && !shares[j]) return fail(AMPH_E_PARAM, "null share array");
  WordArrays arrays;
  for (int j = 0; j < n; ++j) arrays.push_back(arr_in(shares[j], 16));
  arrays.push_back(arr_out(out, 16));
  return run_words(c, W, arrays, false, nullptr, flags, stream, "k_recombine",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     amph::ShareSet set{};
                     for (int j = 0; j < n; ++j) set.s[j] = din[j];
                     return amph::launch_recombine(set, n, cnt, dout[0], c->f, lc);
                   });
}

int amph_recombine_object(amph_ctx* c, const uint8_t* const* shares, int n, const size_t* nbytes,
                          uint8_t* out, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (!shares || !nbytes || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with non-null share and length arrays");
  size_t W;
  bool ragged;
  if (int st = party_words(nbytes, n, &W, &ragged)) return st;
  if (!ragged) return amph_recombine(c, shares, n, AMPH_WORD_WIDTH * W, out, flags, stream);
  const size_t off = AMPH_WORD_WIDTH * (W - 1);
  if (!out) return fail(AMPH_E_PARAM, "null output");
  for (int j = 0; j < n; ++j)
    if (!shares[j] && nbytes[j]) return fail(AMPH_E_PARAM, "null share array");
  if (int st = amph_recombine(c, shares, n, off, out, flags, stream)) return st;
  const uint8_t* tail[AMPH_MAX_PARTIES];
  if (flags & AMPH_F_DEVICE) {
    for (int j = 0; j < n; ++j)
      if (int st = check_dev_words({shares[j]})) return st;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(use_device(c->device));
    TailScratch sc;
    sc.s = s;
    HIP_TRY(hipMallocAsync((void**)&sc.p, 16 * (size_t)n, s));
    if (int st = stage_tail(shares, nbytes, n, off, sc.p, flags, s)) return st;
    for (int j = 0; j < n; ++j) tail[j] = sc.p + 16 * j;
    return amph_recombine(c, tail, n, 16, out + off, flags, stream);
  }
  uint8_t words[16 * AMPH_MAX_PARTIES], res[16];
  if (int st = stage_tail(shares, nbytes, n, off, words, flags, nullptr)) return st;
  for (int j = 0; j < n; ++j) tail[j] = words + 16 * j;
  if (int st = amph_recombine(c, tail, n, 16, res, 0, nullptr)) return st;
  return put_word(out, off, res, flags);
}

int amph_verify(amph_ctx* c, const uint8_t* y, const uint8_t* r, const uint8_t* u,
                const uint8_t* v, const uint8_t* w, size_t words, int64_t* first_fail,
                uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (words && (!y || !r || !u || !v || !w)) return fail(AMPH_E_PARAM, "null input");
  return run_words(c, words, {arr_in(y, 16), arr_in(r, 16), arr_in(u, 16), arr_in(v, 16), arr_in(w, 16)}, true,
                   first_fail, flags, stream, "k_verify",
                   [&](const DevIn& din, const DevOut&, size_t cnt, unsigned long long* ff,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_verify(din[0], din[1], din[2], din[3], din[4], cnt, ff, c->f, lc);
                   });
}

int amph_verify_message(amph_ctx* c, const uint8_t y[16], const uint8_t r[16], const uint8_t u[16],
                        const uint8_t v[16], const uint8_t w[16], char* buf, size_t cap) {
  if (check_ctx(c) || !y || !r || !u || !v || !w) return -AMPH_E_PARAM;
  const u128 Y = ld128(y) % c->p, R = ld128(r) % c->p, V = ld128(v) % c->p;
  const u128 Wv = ld128(w), Uv = ld128(u);
  const u128 aw = mulmod_host(c, Y, R), au = mulmod_host(c, V, R);
  const std::string m = "Verification of secret has failed:\n\t" + dec(Wv) + " = " + dec(ld128(y)) +
                        " * " + dec(ld128(r)) + "   &&   " + dec(Uv) + " = " + dec(ld128(v)) +
                        " * " + dec(ld128(r)) + "\n\t" + dec(Wv) + " = " + dec(aw) +
                        "   &&   " + dec(Uv) + " = " + dec(au);
  if (buf && cap) {
    const size_t k = std::min(cap - 1, m.size());
    std::memcpy(buf, m.data(), k);
    buf[k] = 0;
  }
  return (int)m.size();
}

int amph_convert_share(amph_ctx* c, const uint8_t* masked, const uint8_t* tuples, size_t words,
                       const uint8_t mac_key_le[16], int use_zero, uint8_t* out, uint32_t flags,
                       void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (!mac_key_le) return fail(AMPH_E_PARAM, "null mac key");
  if (words && (!masked || !tuples || !out)) return fail(AMPH_E_PARAM, "null buffer");
  // [alpha] = alpha R mod p, computed once per call on the host
  const W4 alpha = amph::mont_mul(w4_of(ld128(mac_key_le)), amph::r2_word(c->f), c->f);
  return run_words(c, words, {arr_in(masked, 16), arr_in(tuples, 32), arr_out(out, 32)}, false, nullptr, flags,
                   stream, "k_conv",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_convert_share(din[0], din[1], cnt, alpha, use_zero, dout[0], c->f, lc);
                   });
}

int amph_odo_pre(amph_ctx* c, const uint8_t* share_data, size_t share_stride,
                 const uint8_t* masks, const uint8_t* triples, size_t words, uint8_t* oy,
                 uint8_t* orr, uint8_t* ov, uint8_t* omag, uint8_t* oneg, uint32_t flags,
                 void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (share_stride != 16 && share_stride != 32)
    return fail(AMPH_E_PARAM, "share_stride must be 16 or 32");
  if (words && (!share_data || !masks || !triples || !oy || !orr || !ov || !omag || !oneg))
    return fail(AMPH_E_PARAM, "null buffer");
  const int sw = (int)(share_stride / 16);
  return run_words(c, words,
                   {arr_in(share_data, share_stride), arr_in(masks, 64), arr_in(triples, 192), arr_out(oy, 16),
                    arr_out(orr, 16), arr_out(ov, 16), arr_out(omag, 64), arr_out(oneg, 4, 0)},
                   false, nullptr, flags, stream, "k_odo_pre",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_odo_pre(din[0], sw, din[1], din[2], cnt, dout[0], dout[1], dout[2],
                                                 dout[3], (uint32_t*)dout[4], c->f, lc);
                   });
}

int amph_open_diffs(amph_ctx* c, const uint8_t* const* mags, const uint8_t* const* negs, int n,
                    size_t n_pairs, uint8_t* out, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (!mags || !negs || n < 1 || n > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  if (n_pairs % 2) return fail(AMPH_E_LEN, "n_pairs must be 2 * words");
  const size_t W = n_pairs / 2;
  if (W && !out) return fail(AMPH_E_PARAM, "null output");
  for (int j = 0; j < n; ++j)
    if (W && (!mags[j] || !negs[j])) return fail(AMPH_E_PARAM, "null diff array");
  WordArrays arrays = diff_arrays(mags, negs, n);
  arrays.push_back(arr_out(out, 64));
  return run_words(c, W, arrays, false, nullptr, flags, stream, "k_open",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_open_diffs(diff_set(din, n), n, cnt, dout[0], c->f, lc);
                   });
}

int amph_odo_post(amph_ctx* c, const uint8_t* opened, const uint8_t* triples, size_t words,
                  int is_player0, uint8_t* ow, uint8_t* ou, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (words && (!opened || !triples || !ow || !ou)) return fail(AMPH_E_PARAM, "null buffer");
  return run_words(c, words, {arr_in(opened, 64), arr_in(triples, 192), arr_out(ow, 16), arr_out(ou, 16)}, false,
                   nullptr, flags, stream, "k_odo_post",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_odo_post(din[0], din[1], cnt, is_player0, dout[0], dout[1], c->f, lc);
                   });
}

int amph_open_post(amph_ctx* c, const uint8_t* const* mags, const uint8_t* const* negs, int n,
                   const uint8_t* triples, size_t words, int is_player0, uint8_t* ow, uint8_t* ou,
                   uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (!mags || !negs || n < 1 || n > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  if (words && (!triples || !ow || !ou)) return fail(AMPH_E_PARAM, "null buffer");
  for (int j = 0; j < n; ++j)
    if (words && (!mags[j] || !negs[j])) return fail(AMPH_E_PARAM, "null diff array");
  WordArrays arrays = diff_arrays(mags, negs, n);
  for (const WordArray& x : {arr_in(triples, 192), arr_out(ow, 16), arr_out(ou, 16)}) arrays.push_back(x);
  return run_words(c, words, arrays, false, nullptr, flags, stream, "k_open_post",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_open_post(diff_set(din, n), n, din[2 * n], cnt, is_player0, dout[0],
                                                   dout[1], c->f, lc);
                   });
}

int amph_to_gfp(amph_ctx* c, const uint8_t* in, size_t words, uint8_t* out, uint32_t flags,
                void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (words && (!in || !out)) return fail(AMPH_E_PARAM, "null buffer");
  return run_words(c, words, {arr_in(in, 16), arr_out(out, 16)}, false, nullptr, flags, stream, "k_to_gfp",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_to_gfp(din[0], cnt, dout[0], c->f, lc);
                   });
}

int amph_from_gfp(amph_ctx* c, const uint8_t* in, size_t words, uint8_t* out, uint32_t flags,
                  void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (words && (!in || !out)) return fail(AMPH_E_PARAM, "null buffer");
  return run_words(c, words, {arr_in(in, 16), arr_out(out, 16)}, false, nullptr, flags, stream, "k_from_gfp",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_from_gfp(din[0], cnt, dout[0], c->f, lc);
                   });
}

int amph_mask_words(amph_ctx* c, const uint8_t* secrets, const uint8_t* masks, size_t words,
                    uint8_t* out, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_HOST_IO_ENTRY(flags);
  if (words && (!secrets || !masks || !out)) return fail(AMPH_E_PARAM, "null buffer");
  return run_words(c, words, {arr_in(secrets, 16), arr_in(masks, 16), arr_out(out, 16)}, false, nullptr, flags,
                   stream, "k_mask_words",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_mask_words(din[0], din[1], cnt, dout[0], c->f, lc);
                   });
}

int amph_mask_word_host(amph_ctx* c, const uint8_t secret[16], const uint8_t mask[16], uint8_t out[16]) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (!secret || !mask || !out) return fail(AMPH_E_PARAM, "null word");
  const u128 s = ld128(secret) % c->p, m = ld128(mask) % c->p;
  u128 d = s - m;  // mod 2^128; the true difference (s - m) mod p is < p < 2^128
  if (s < m) d += c->p;
  const W4 x = amph::mont_mul(w4_of(d), amph::r2_word(c->f), c->f);  // d R mod p, reduced
  for (int i = 0; i < 4; ++i) std::memcpy(out + 4 * i, &x.v[i], 4);
  return AMPH_OK;
}

int amph_synth_odos(amph_ctx* c, uint64_t seed, int n, size_t words, uint8_t* const* out_fields,
                    uint8_t* out_plain_y, int64_t fault_index, int noncanon_permille,
                    void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (!out_fields || n < 1 || n > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  amph::OutSet set{};
  for (int k = 0; k < 5; ++k)
    for (int j = 0; j < n; ++j) {
      if (words && !out_fields[k * n + j]) return fail(AMPH_E_PARAM, "null output field");
      set.f[k][j] = (uint4*)out_fields[k * n + j];
    }
  HIP_TRY(use_device(c->device));
  hipError_t e = amph::launch_synth_odos(set, n, words, seed, (uint4*)out_plain_y, fault_index,
                                         noncanon_permille, c->f, cfg(c, (hipStream_t)stream, words));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_synth");
}

int amph_stream_probe(amph_ctx* c, const amph_odo* odos, int n, const uint8_t* secrets, size_t words,
                      uint8_t* out, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  size_t W;
  if (int st = odo_words(odos, n, &W)) return st;
  if (words > W) return fail(AMPH_E_LEN, "more words than the ODO arrays hold");
  if (words && (!secrets || !out)) return fail(AMPH_E_PARAM, "null secrets/output");
  if (int st = check_dev_odos(odos, n)) return st;
  if (int st = check_dev_words({secrets, out})) return st;
  HIP_TRY(use_device(c->device));
  hipError_t e = amph::launch_stream_probe(odo_set(odos, n), n, words, (const uint4*)secrets, (uint4*)out,
                                           cfg(c, (hipStream_t)stream, words));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_stream_probe");
}

int amph_synth_words(amph_ctx* c, uint64_t seed, size_t count, uint8_t* out, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (count && !out) return fail(AMPH_E_PARAM, "null output");
  HIP_TRY(use_device(c->device));
  hipError_t e = amph::launch_synth_words((uint4*)out, count, seed, c->f, cfg(c, (hipStream_t)stream, count));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_synth_words");
}

}  // extern "C"
