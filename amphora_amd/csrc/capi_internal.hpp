// Internals shared by the units of the C ABI (capi_*.hip -- capi_ctx,
// capi_pipeline, capi_words, capi_text, capi_party, parties_session,
// client_session, clients_session and capi_batch, the many-objects-per-call
// families): the context, the error and device helpers, the word-array
// pipeline's types, the buffers of one-shot host calls and the one host image
// of the many-objects calls.  Everything here lives in one namespace of hidden
// visibility: the library exports only what include/amphora.h and its
// extension headers include/amphora_wire_batch.h,
// include/amphora_upload_batch.h, include/amphora_respond_batch.h,
// include/amphora_exchange_batch.h, include/amphora_party_batch.h,
// include/amphora_client_session.h, include/amphora_client_batch.h and
// include/amphora_client_bodies.h declare.
//
// Host-pointer calls stream the word arrays through the device in batches
// (ctx->batch_words, default 4 Mi words): per batch the inputs go HtoD on the
// copy-in stream, the kernel runs on the kernel stream, the outputs come back
// DtoH on the copy-out stream; three device-side slots let batch k+1's copies
// overlap batch k's kernel and batch k-1's copy out (run_batched).  Verify
// failures are reported per batch into a device array of first-fail words,
// read back once at the end.  Device-pointer calls (AMPH_F_DEVICE) launch
// straight onto the caller's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include <atomic>
#include <memory>
#include <thread>

#include "../../include/amphora.h"
#include "../../include/amphora_wire_batch.h"
#include "../../include/amphora_upload_batch.h"
#include "../../include/amphora_respond_batch.h"
#include "../../include/amphora_exchange_batch.h"
#include "../../include/amphora_party_batch.h"
#include "../../include/amphora_client_session.h"
#include "../../include/amphora_client_batch.h"
#include "../../include/amphora_client_bodies.h"
#include "host_stream.hpp"
#include "kernels.hpp"
#include "wiretiles.hpp"

namespace capi __attribute__((visibility("hidden"))) {
using amph::Fp;
using amph::W4;

// The thread-locals stay private to the unit that defines them and are
// reached through functions: a constant-initialised extern thread_local of
// hidden visibility is read through a wrapper whose init hook the linker
// leaves unresolved, and the first access from another unit jumps to null.
int fail(int status, const std::string& msg);
const std::string& last_error();   // what fail() recorded on this thread
void drop_launch_timing();         // forget a pending amph_time_next_launch
int hip_fail(hipError_t e, const char* what);

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);   \
  } while (0)

// The context's device for this thread's next HIP calls: hipSetDevice only
// when the thread's current device differs (hipGetDevice reads thread-local
// state; the set is what a thread's first HIP call pays for).
hipError_t use_device(int device);

typedef unsigned __int128 u128;

inline u128 ld128(const uint8_t* b) {
  uint64_t lo, hi;
  std::memcpy(&lo, b, 8);
  std::memcpy(&hi, b + 8, 8);
  return ((u128)hi << 64) | lo;
}

inline W4 w4_of(u128 x) {
  return W4{{(uint32_t)x, (uint32_t)(x >> 32), (uint32_t)(x >> 64), (uint32_t)(x >> 96)}};
}

inline u128 u128_of(const W4& w) {
  return ((u128)w.v[3] << 96) | ((u128)w.v[2] << 64) | ((u128)w.v[1] << 32) | w.v[0];
}

inline std::string dec(u128 x) {
  if (x == 0) return "0";
  char buf[48];
  int n = 0;
  while (x) {
    buf[n++] = (char)('0' + (int)(x % 10));
    x /= 10;
  }
  std::string s(buf, n);
  std::reverse(s.begin(), s.end());
  return s;
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace capi
using namespace capi;  // this header is for the capi_*.hip units only

struct amph_ctx {
  int device = 0;
  Fp f{};
  u128 p = 0, r = 0, rinv = 0;
  std::mutex mu;
  size_t batch_words = (size_t)4 << 20;
  int grid_cap = 0;
  int block = 0;  // 0 = by size (block_for)
  // host-pointer path: kSlots batches in flight, one stream each
  static constexpr int kSlots = 3;
  struct Slot {
    DevBuf dev;
    amph::PinnedBuf hin, hout;
    hipEvent_t in_done = nullptr, k_done = nullptr, out_done = nullptr;
    bool busy = false;  // hout holds outputs not yet copied to the caller
    bool used = false;  // the slot has a batch in this call (its events are live)
    size_t base = 0, cnt = 0;
  };
  hipStream_t streams[kSlots] = {};  // host path: HtoD, kernels, DtoH
  Slot slots[kSlots];
  std::vector<amph_ctx*> sub;  // amph_ctx_create_multi: one context per device
  // a sub-context's own long-lived thread (run_sharded posts its shards here)
  std::unique_ptr<amph::DeviceWorker> worker;
  DevBuf ff;  // per-batch first-fail words (host path)
  DevBuf tail;  // small scratch for the partial last unit of codec calls
  DevBuf wire;  // host-mode staging of the wire-text calls (texts, secrets, outputs, verdicts)
  // the many-objects wire-text calls (amphora_wire_batch.h): the page-locked
  // image their staged host mode gathers into and scatters from, and the
  // hipMemcpy calls that moved it (amph_wire_batch_copies)
  amph::PinnedBuf wire_img;
  std::atomic<uint64_t> wire_copies{0};
  std::atomic<uint64_t> upload_copies{0};  // the same of amphora_upload_batch.h's calls (amph_upload_batch_copies)
  std::atomic<uint64_t> respond_copies{0};  // and of amphora_respond_batch.h's (amph_respond_batch_copies)
  std::atomic<uint64_t> exchange_copies{0};  // and of amphora_exchange_batch.h's (amph_exchange_batch_copies)
  std::atomic<uint64_t> clients_copies{0};  // and of amphora_client_batch.h's host-mode calls (amph_clients_copies)
  DevBuf xstage;  // host-mode staging of the exchange codec calls
  DevBuf xdev;    // device-mode scan scratch of the exchange codec calls
  hipEvent_t xdev_done = nullptr;  // the last device-mode exchange call's kernels
  // small host calls (run_small): one page-locked arena the kernels read and
  // write in place, and device verdict words kept at kNoFail between calls
  size_t small_bytes = (size_t)2 << 20;
  amph::PinnedBuf small;
  DevBuf small_ff;
  DevBuf seg;  // packed host calls (run_packed): the device offsets table, then the verdict array
  bool small_ff_dirty = true;
  std::unique_ptr<amph::CopyPool> pool;
  // party sessions' device buffers, kept after amph_party_free for the next
  // session: a server runs one session per request, and hipMalloc / hipFree of
  // its gigabytes cost tens of microseconds per buffer (hipFree synchronises
  // the device) -- best fit, at most kPartyPoolMax buffers, freed with the context
  std::vector<DevBuf> party_pool;
  size_t pool_cap_bytes = (size_t)32 << 30;  // AMPH_PARTY_POOL_BYTES
  std::atomic<uint64_t> launches{0};      // amph_ctx_stats
  std::atomic<uint64_t> worker_tasks{0};
};

// The client session for K secrets (include/amphora_client_batch.h,
// clients_session.hip; the body calls of include/amphora_client_bodies.h,
// clients_bodies.hip, hand a party in on the same session).
struct amph_clients {
  amph_ctx* c = nullptr;
  size_t K = 0, T = 0;
  int n = 0;
  bool dev = false;
  hipStream_t dstream = nullptr;  // device mode: the stream of the latest call
  std::vector<uint64_t> woff, foff, uoff;  // word (K + 1), field text (K) and framed text (K) offsets
  size_t field_chars = 0, used_chars = 0, upload_chars = 0;  // used: the end of the last field text
  DevBuf mem;
  amph::PinnedBuf tables_host;  // device mode: the image the tables are uploaded from
  amph::SumSet sums{};
  // device tables, contiguous in this order (one upload): word, field text, framed text offsets
  uint64_t *d_woff = nullptr, *d_foff = nullptr, *d_uoff = nullptr;
  unsigned long long* d_bad = nullptr;  // K words: min over the parties, the packed calls' encoding
  // device mode, the body calls: the device starts[5][K] (rewritten in stream order by each call) and the
  // page-locked images it is uploaded from, one per party slot (in tables_host, behind the tables)
  uint64_t *d_starts = nullptr, *starts_host = nullptr;
  std::vector<unsigned long long> bad_host;  // host mode: the same, as the party calls returned it
  uint32_t have = 0;  // bit j: party j's texts are in the sums
  bool finished = false;
  ~amph_clients() { tables_host.release(); }
};

namespace capi __attribute__((visibility("hidden"))) {

// what every call on a client batch session checks first (clients_session.hip)
int clients_check(amph_clients* p, bool dev, bool open);

// a context allocation that frees the pooled party-session buffers and tries
// once more when memory runs out (capi_ctx.hip)
size_t pool_bytes(const amph_ctx* c);
hipError_t dev_ensure(amph_ctx* c, DevBuf& b, size_t bytes);
// the party sessions' buffers (capi_party.hip; c->mu held): pool_put hands one
// back to the context's pool -- at most kPartyPoolMax buffers and
// c->pool_cap_bytes bytes, the smallest dropped first; pool_ensure makes b
// hold at least `bytes`: kept, or the best-fitting pooled buffer, or a new
// allocation (after freeing the pool if memory ran out)
constexpr size_t kPartyPoolMax = 16;
void pool_put(amph_ctx* c, DevBuf& b);
hipError_t pool_ensure(amph_ctx* c, DevBuf& b, size_t bytes);
inline size_t b64_chars(size_t nbytes) { return 4 * ((nbytes + 2) / 3); }
u128 mulmod_host(const amph_ctx* c, u128 a, u128 b);  // a < p
amph::LaunchCfg cfg(amph_ctx* c, hipStream_t s, size_t words);
inline int check_ctx(amph_ctx* c) { return c ? AMPH_OK : fail(AMPH_E_PARAM, "null context"); }
// where a multi-device context runs the calls that are not sharded: its first device's context
inline amph_ctx* first_device(amph_ctx* c) { return c->sub.empty() ? c : c->sub[0]; }
inline const amph_ctx* first_device(const amph_ctx* c) { return c->sub.empty() ? c : c->sub[0]; }

// ---- word-array calls (capi_pipeline.hip) --------------------------------------
// A word-array call is described by its input and output arrays, each with a
// per-word byte size; the kernel launcher receives device pointers of one
// batch (host mode) or the caller's own (AMPH_F_DEVICE).
struct WordArray {
  uint8_t* host;                          // the caller's pointer; only outputs are written through it
  size_t bytes_per_word;
  // AMPH_F_DEVICE: 16 for word arrays (read and written as 16-byte vectors,
  // global_load/store_dwordx4), 8 for 24-character base64 records (8-byte
  // vectors), 0 for the 4-byte sign words, which are not checked
  int dev_align = 16;
  bool out = false;
  size_t base = 0;                        // words into the array where this call starts
  const amph_host_array* io = nullptr;    // AMPH_F_HOST_IO: the callbacks (host unused)
};
inline WordArray arr_in(const void* p, size_t bytes_per_word, int dev_align = 16, size_t base = 0) {
  return WordArray{(uint8_t*)const_cast<void*>(p), bytes_per_word, dev_align, false, base};
}
inline WordArray arr_out(void* p, size_t bytes_per_word, int dev_align = 16) {
  return WordArray{(uint8_t*)p, bytes_per_word, dev_align, true};
}
typedef std::vector<WordArray> WordArrays;
typedef std::vector<const uint4*> DevIn;
typedef std::vector<uint4*> DevOut;
// The launch of one batch -- called once per batch (host mode) or once (device
// mode) -- as a non-owning reference to the entry point's callable, which
// outlives the call: the pipeline is ordinary functions compiled once.
class Launch {
 public:
  template <class F>
  Launch(const F& f)
      : f_(&f), call_([](const void* f, const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long* ff,
                         const amph::LaunchCfg& lc) { return (*(const F*)f)(din, dout, cnt, ff, lc); }) {}
  hipError_t operator()(const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long* ff,
                        const amph::LaunchCfg& lc) const {
    return call_(f_, din, dout, cnt, ff, lc);
  }

 private:
  const void* f_;
  hipError_t (*call_)(const void*, const DevIn&, const DevOut&, size_t, unsigned long long*, const amph::LaunchCfg&);
};

// AMPH_F_HOST_IO for the calling thread's current ABI call: set by the entry
// point (HostIoScope), turned into WordArray::io by run_batched before any
// work leaves this thread.
struct HostIoScope {
  explicit HostIoScope(uint32_t flags);
  ~HostIoScope();
};

// Entry of a call that accepts AMPH_F_HOST_IO / one that refuses it.
#define AMPH_HOST_IO_ENTRY(flags)                                                      \
  if (((flags) & AMPH_F_HOST_IO) && ((flags) & AMPH_F_DEVICE))                         \
    return fail(AMPH_E_PARAM, "AMPH_F_HOST_IO and AMPH_F_DEVICE exclude each other");  \
  HostIoScope host_io_scope_(flags)
#define AMPH_NO_HOST_IO(flags) \
  if ((flags) & AMPH_F_HOST_IO) return fail(AMPH_E_PARAM, "AMPH_F_HOST_IO is not accepted by this call")

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Device-pointer word arrays are read and written as 16-byte vectors
// (global_load/store_dwordx4), so every one must be 16-byte aligned.
int check_dev_words(std::initializer_list<const void*> ptrs);
// device-mode first-fail: reset to the sentinel on the caller's stream,
// unless the caller accumulates (AMPH_F_ACCUMULATE: min-combine into it)
int reset_ff_dev(int64_t* ff, uint32_t flags, hipStream_t s);

// Host mode of a word-array call: host-io descriptors, then a multi-device
// context's shards, then a small call, then the batched pipeline.
int run_batched(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
                int64_t* first_fail, const Launch& launch, size_t ff_scale = 1);

// One word-array call in either mode; `arrays` lists inputs and outputs in the
// order device mode checks their alignment, `launch` sees the inputs as din[]
// and the outputs as dout[] in that order.
//   AMPH_F_DEVICE: the alignment checks come before the device is selected (a
// caller without a GPU gets AMPH_E_PARAM for a misaligned pointer), then the
// verdict word is reset and `launch` runs once over the caller's pointers on
// the caller's stream -- no context mutex; a failure is reported as `kernel`.
//   Host mode: under the context mutex, run_batched.
int run_words(amph_ctx* c, size_t words, const WordArrays& arrays, bool with_ff, int64_t* first_fail,
              uint32_t flags, void* stream, const char* kernel, const Launch& launch);

// ---- packed calls (capi_pipeline.hip) --------------------------------------------
// The launch of one batch of a packed (segmented) call: Launch's arguments
// with the batch's first global word, the device copy of the offsets table
// and the call's device verdict array (one word per object).
typedef std::function<hipError_t(const DevIn& din, const DevOut& dout, size_t cnt, size_t base,
                                 const uint64_t* offsets, unsigned long long* ff, const amph::LaunchCfg& lc)>
    SegLaunch;
// Host mode of a packed call, under the context mutex: `offsets` (validated by
// the caller, n_objects + 1 host words, offsets[n_objects] = words) goes to
// the device once, the verdict array stays there across the call's batches
// and is read back once.  A call that fits the small-call arena runs there
// (table and verdicts included), any other through the batched pipeline.
// first_fail[o] = -1 or object o's smallest failing local index;
// AMPH_E_VERIFY (amph_last_error names the first failing object) if any failed.
int run_packed(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, const uint64_t* offsets,
               size_t n_objects, int64_t* first_fail, const SegLaunch& launch);

// ---- one-shot host calls (capi_pipeline.hip) -----------------------------------
// Results of a one-shot host call: wait for the stream, then copy with
// blocking hipMemcpy (kPageableRule, above read_back's definition).
struct ReadBack {
  void* dst;
  const void* src;
  size_t bytes;
};
hipError_t read_back(hipStream_t s, std::initializer_list<ReadBack> copies);

// the context's own stream k (host mode), created on first use
int host_stream(amph_ctx* c, int k, hipStream_t* s);
bool small_call(const amph_ctx* c, size_t bytes);
// device bytes of arrays carved by Stager::take
size_t carve_bytes(std::initializer_list<size_t> sizes);

// The buffers of a one-shot host call (one launch, no batching): run_small,
// the wire-text calls and the exchange codec.  Small: the page-locked arena
// (capi_pipeline.hip), plain memcpy in and out, the context's device verdict words
// (kept at kNoFail between calls), one synchronisation.  Staged: everything
// carved from one per-context device buffer (grown with hipMalloc, held under
// the context mutex), each input copied with a blocking hipMemcpy while the
// context's stream is idle (kPageableRule) and the results read back after
// the kernel.  Two earlier forms of the staged path failed:
//   * stream-ordered hipMallocAsync staging with pageable hipMemcpyAsync: in
//     a fresh process the first wire-text call intermittently saw the first
//     text unit unwritten;
//   * two contexts on one device calling at the same time got overlapping
//     hipMallocAsync buffers: each party's exchange text came back empty or
//     overwritten (tools/c1_native, two party threads).
struct Stager {
  amph_ctx* c = nullptr;
  hipStream_t s = nullptr;
  bool small = false;
  int n_ff = 0;
  unsigned long long* fl = nullptr;  // the device verdict words (staged: after arm)
  uint8_t *base = nullptr, *dev_base = nullptr;
  size_t off = 0;
  // `bytes` of arena when small (plus 256 for the verdict words at its head);
  // dev_bytes of *dev: the scratch of a small call, everything of a staged one
  int begin(amph_ctx* ctx, hipStream_t stream, bool use_small, size_t bytes, int verdict_words,
            DevBuf* dev = nullptr, size_t dev_bytes = 0, const char* what = "");
  uint8_t* take(size_t bytes) {
    uint8_t* p = base + off;
    off += align256(bytes ? bytes : 16);
    return p;
  }
  // the call's device-only scratch (at most one): never in the arena
  void* scratch(size_t bytes) { return small ? dev_base : take(bytes); }
  // one word the kernel itself writes for the host (a call without verdict
  // words): straight into the arena head, or a staged word
  unsigned long long* result_word();
  hipError_t put(void* dst, const void* src, size_t bytes);
  // once, before the launch: a staged call's verdict words, reset on the stream
  int arm();
  // after the launch: the verdict words into v (small: to the arena head by
  // one copy kernel -- none without verdict words -- and ONE synchronisation)
  // and `outs` to the caller
  int finish(int64_t* v, std::initializer_list<ReadBack> outs);
  // outputs a call copies only once it has looked at the verdict
  int fetch(std::initializer_list<ReadBack> outs);
  int launch_failed(hipError_t e, const char* what);
};

// the verdict word of an exchange decode (`pairs` FactorPairs expected in
// `len` characters) as the call's status and message (capi_text.hip)
int decode_status(int64_t bad, size_t len, size_t pairs, int64_t* bad_index);
// the device-mode exchange calls' scratch: `bytes` of the context's buffer,
// behind the previous such call's kernels on `s` (capi_text.hip; call under
// the context mutex and record c->xdev_done after the launches)
int dev_scratch(amph_ctx* c, size_t bytes, hipStream_t s, void** p);

// ---- the base64 wire texts (capi_text.hip; the batch calls of capi_batch.hip) ----
extern const char* const kOdoFieldNames[5];
const char* b64_field(const amph_odo_b64& o, int k);  // field k's text, in ODO order
// 1..16 parties and their array: what every wire-text call checks first
int check_parties(const amph_odo_b64* odos, int n);
// AMPH_E_PARAM with the wire-text calls' message for a bad_char verdict,
// (5 party + field) * nchars + offset
int wire_bad_message(int64_t bad, size_t nchars);

// The verdict words of a many-objects wire-text call (first-fail array, then
// bad-character array, K words each) as the caller's entries and the call's
// status: the packed calls of capi_batch.hip and the K-secret client session
// (clients_session.hip) report alike.
inline int wire_batch_status(const unsigned long long* v, size_t K, const uint64_t* woff, int64_t* first_fail,
                             int64_t* bad_char) {
  size_t nbad = 0, nfail = 0, fb = 0, ff = 0;
  for (size_t o = 0; o < K; ++o) {
    const bool bad = v[K + o] != amph::kNoFail, failed = !bad && v[o] != amph::kNoFail;
    if (bad && !nbad++) fb = o;
    if (failed && !nfail++) ff = o;
    bad_char[o] = bad ? (int64_t)v[K + o] : -1;
    first_fail[o] = failed ? (int64_t)v[o] : -1;
  }
  if (nbad) {
    const size_t nc = amph::wire_text_chars(woff[fb + 1] - woff[fb]), f = (size_t)v[K + fb] / nc;
    return fail(AMPH_E_PARAM, "object " + std::to_string(fb) + ": Illegal base64 character at index " +
                                  std::to_string((size_t)v[K + fb] % nc) + " of party " + std::to_string(f / 5) +
                                  "'s " + kOdoFieldNames[f % 5] + " (" + std::to_string(nbad) + " of " +
                                  std::to_string(K) + " objects hold an illegal character)");
  }
  if (nfail)
    return fail(AMPH_E_VERIFY, "Verification of secret has failed: object " + std::to_string(ff) + " at word " +
                                   std::to_string(v[ff]) + " (" + std::to_string(nfail) + " of " +
                                   std::to_string(K) + " objects failed)");
  return AMPH_OK;
}

// ---- the host image of the many-objects calls -----------------------------------
// Host mode of every call of capi_batch.hip and of the K-secret client
// session moves ONE image to the device and one back, whatever the object
// count, around ONE launch (the exchange codec's: one fixed sequence of
// launches): 256-aligned regions, all the inputs (tables first) before all
// the outputs, the verdict words last.
//   Small (the image fits the small-call arena): it is built in the arena and
// the kernel reads and writes it in place; the verdict words stay in device
// memory (c->seg: atomics) while the kernel runs and come to the arena by a
// copy kernel before the call's one synchronisation, as run_packed_small.
// No host-device copy.
//   Staged: the image is built in c->wire_img (page-locked) and mirrored in
// c->wire; one blocking copy of the inputs while the stream is idle
// (kPageableRule), one of the outputs and verdicts after the synchronisation,
// each counted in the family's copy counter.
// The context's mutex is held from open() to the image's end of life; a
// caller that already holds it hands its lock over in `lock` before open().
struct BatchImage {
  amph_ctx* c = nullptr;
  hipStream_t s = nullptr;
  bool small = false;
  size_t in_bytes = 0, total = 0;  // the inputs are [0, in_bytes), the outputs [in_bytes, total)
  size_t verd = 0, n_verd = 0;     // the verdict words' offset and count
  const char* verd_what = "";
  uint8_t *himg = nullptr, *dimg = nullptr;
  unsigned long long* dverd = nullptr;  // the verdict words the kernel writes
  std::atomic<uint64_t>* copies = nullptr;
  std::unique_lock<std::mutex> lock;

  // Regions, in the image's order: every in() before the first out(), verdicts() last.
  size_t in(size_t bytes) {
    const size_t at = in_bytes;
    total = in_bytes += align256(bytes);
    return at;
  }
  size_t out(size_t bytes) {
    const size_t at = total;
    total += align256(bytes);
    return at;
  }
  void verdicts(size_t words, const char* what) {
    n_verd = words;
    verd_what = what;
    verd = out(8 * words);
  }

  // `family` names the staged buffers in an AMPH_E_NOMEM message
  int open(amph_ctx* ctx, std::atomic<uint64_t> amph_ctx::*counter, const char* family) {
    c = first_device(ctx);
    copies = &(c->*counter);
    if (!lock.owns_lock()) lock = std::unique_lock<std::mutex>(c->mu);
    HIP_TRY(use_device(c->device));
    if (int st = host_stream(c, 0, &s)) return st;
    small = small_call(c, total);
    if (small) {
      if (c->small.ensure(total + 256) != hipSuccess) return fail(AMPH_E_NOMEM, "small-call arena");
      if (n_verd && dev_ensure(c, c->seg, 8 * n_verd) != hipSuccess) return fail(AMPH_E_NOMEM, verd_what);
      himg = dimg = (uint8_t*)c->small.p;
      dverd = (unsigned long long*)c->seg.p;
    } else {
      if (c->wire_img.ensure(total) != hipSuccess) return fail(AMPH_E_NOMEM, std::string(family) + " batch image");
      if (dev_ensure(c, c->wire, total) != hipSuccess) return fail(AMPH_E_NOMEM, std::string(family) + " staging");
      himg = (uint8_t*)c->wire_img.p;
      dimg = (uint8_t*)c->wire.p;
      dverd = (unsigned long long*)(dimg + verd);
    }
    return AMPH_OK;
  }
  uint8_t* host(size_t off) const { return himg + off; }
  uint8_t* dev(size_t off) const { return dimg + off; }
  const uint64_t* dev_table(size_t off) const { return (const uint64_t*)(dimg + off); }
  const unsigned long long* verdict_words() const { return (const unsigned long long*)(himg + verd); }

  // staged only: bytes [from, to) of the image to the device or back, as one
  // blocking, counted copy -- page-locked image, idle stream (kPageableRule)
  int move(size_t from, size_t to, hipMemcpyKind kind) {
    if (small) return AMPH_OK;
    uint8_t *dst = kind == hipMemcpyHostToDevice ? dimg : himg, *src = kind == hipMemcpyHostToDevice ? himg : dimg;
    HIP_TRY(hipMemcpy(dst + from, src + from, to - from, kind));
    copies->fetch_add(1, std::memory_order_relaxed);
    return AMPH_OK;
  }

  // the inputs are in place: to the device, the verdict words reset
  int upload() {
    if (int st = move(0, in_bytes, hipMemcpyHostToDevice)) return st;
    if (n_verd) HIP_TRY(hipMemsetAsync(dverd, 0x7F, 8 * n_verd, s));
    return AMPH_OK;
  }

  // after the call's one launch (`e`): outputs and verdict words are in host(...)
  int finish(hipError_t e, const char* kernel) {
    if (e == hipSuccess && small && n_verd)
      e = amph::launch_take_array(dverd, (unsigned long long*)(himg + verd), n_verd, s);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s);
      return hip_fail(e, kernel);
    }
    HIP_TRY(hipStreamSynchronize(s));
    return move(in_bytes, total, hipMemcpyDeviceToHost);
  }
};

}  // namespace capi
