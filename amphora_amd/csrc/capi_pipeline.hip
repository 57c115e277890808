// How the C ABI moves word arrays through the device (capi_internal.hpp):
// the batched, small and sharded runners of host-pointer calls, the
// dispatcher of the per-word entry points, and the buffers of one-shot host
// calls.
#include "capi_internal.hpp"

namespace capi __attribute__((visibility("hidden"))) {
namespace {
thread_local bool g_host_io = false;
}  // namespace
HostIoScope::HostIoScope(uint32_t flags) { g_host_io = (flags & AMPH_F_HOST_IO) != 0; }
HostIoScope::~HostIoScope() { g_host_io = false; }

namespace {
// the staging copy of `words` words from word `word` of input x into dst
amph::CopyTask copy_in(const WordArray& x, size_t word, size_t words, void* dst) {
  const size_t off = (x.base + word) * x.bytes_per_word, bytes = words * x.bytes_per_word;
  if (x.io) return amph::CopyTask{dst, nullptr, bytes, x.io, off, false};
  return amph::CopyTask{dst, x.host + off, bytes};
}
amph::CopyTask copy_out(const WordArray& x, size_t word, size_t words, const void* src) {
  const size_t off = (x.base + word) * x.bytes_per_word, bytes = words * x.bytes_per_word;
  if (x.io) return amph::CopyTask{nullptr, src, bytes, x.io, off, true};
  return amph::CopyTask{x.host + off, src, bytes};
}
int io_failed() { return fail(AMPH_E_PARAM, "a host array callback (AMPH_F_HOST_IO) failed"); }

}  // namespace

// kPageableRule -- the ordering rule every host<->device copy here follows:
//
//   hipMemcpyAsync is used ONLY with page-locked host memory (the batched
//   pipeline's slot buffers, or caller buffers is_pinned_host() reports as
//   registered).  Pageable host memory moves with a blocking hipMemcpy,
//   issued only once the context stream that produces / consumes the device
//   side has been synchronised.
//
// Why: HIP defines an async copy of pageable memory only as "performed
// synchronously" (hip_runtime_api.h, hipMemcpyAsync @note) -- a host-staged
// transfer, not the stream-ordered copy CUDA code assumes -- so its order
// against the kernels of a non-blocking stream is not a guarantee this
// library may build on.  Round 2 saw that order fail once in each direction,
// both times in a one-shot call on a non-blocking context stream:
//   * DtoH (1e4fc5f): a pageable verdict word on the stack, hipMemcpyAsync'd
//     after the kernel that writes it, held the value from before the kernel;
//   * HtoD (9513c3e): base64 text hipMemcpyAsync'd from pageable memory into
//     hipMallocAsync staging on the same stream was seen by the kernel with
//     its first 16-character unit (the head of the first copy) unwritten.
// tests/test_host_ordering.py checks the rule statically over the capi units and
// runs a fresh process's first wire-text calls on the GPU.
//
// Results of a one-shot host call: wait for the stream, then copy with
// blocking hipMemcpy.
hipError_t read_back(hipStream_t s, std::initializer_list<ReadBack> copies) {
  hipError_t e = hipStreamSynchronize(s);
  for (const ReadBack& r : copies)
    if (e == hipSuccess && r.bytes) e = hipMemcpy(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost);
  return e;
}

namespace {
int host_threads() {
  if (const char* t = std::getenv("AMPH_HOST_THREADS")) return std::max(1, std::atoi(t));
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(8u, hw ? hw / 2 : 1u));
}

int run_sharded(amph_ctx* g, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
                int64_t* first_fail, const Launch& launch, size_t ff_scale);

// Batch size of a host call: at most ctx->batch_words, and small enough that
// the call has about 8 batches -- so copies in, kernels and copies out of
// consecutive batches overlap -- but not below 32 MiB of traffic per batch
// (each batch costs a few events and copy launches).  A 4 Mi-word call at 3
// parties used to be ONE batch, every stage back to back: pageable odo_pre
// 43.6 -> 25.7 ms, open_post 48.0 -> 32.8, mask_input 30.8 -> 22.5 with
// 512 Ki-word batches (tools/host_rate_probe.py, profiles/r03_host_batches.jsonl);
// C5's 32 Mi-word calls keep their 4 Mi-word batches.
size_t batch_for(const amph_ctx* c, size_t words, size_t bytes_per_word) {
  constexpr size_t kMinBatchBytes = (size_t)32 << 20;
  const size_t floor_words = std::max<size_t>(1, kMinBatchBytes / std::max<size_t>(1, bytes_per_word));
  const size_t eighth = (words + 7) / 8;
  return std::max<size_t>(1, std::min({words, c->batch_words, std::max(eighth, floor_words)}));
}

// Streams `words` through the device in batches of ctx->batch_words, one
// HIP stream per engine: streams[0] carries every HtoD copy in batch order,
// streams[1] the kernels, streams[2] every DtoH copy.  kSlots device slots
// (inputs + outputs of one batch each) rotate; events order the slot reuse
// on the GPU (batch b's HtoD waits for the kernel of batch b - kSlots, its
// kernel for its HtoD and for the DtoH of batch b - kSlots, its DtoH for its
// kernel), so the copy-in engine streams batch after batch at the link's
// rate while kernels and copies out overlap it (with one stream per slot the
// slots' copies shared the link, finished together, and the link idled while
// their kernels and copies out drained: 2-4 ms every third batch in the
// rocprofv3 memory-copy trace of a C5 step).  The CPU only
// waits to reuse a page-locked staging slot: pageable inputs are copied into
// one by CPU threads once its previous HtoD is done, pageable outputs out of
// one once its previous DtoH is done.  Page-locked caller buffers are DMA'd
// directly.  Verify failures land in one device word per batch; the smallest
// global index is reported.  A kernel reports its failure index in units of
// 1/ff_scale of a batch word (the base64 stream decode: a character offset,
// 16 characters per batch word), so batch b's base is b * bw * ff_scale.
int run_batched_impl(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
                     int64_t* first_fail, const Launch& launch, size_t ff_scale) {
  if (first_fail) *first_fail = -1;
  if (words == 0) return AMPH_OK;
  constexpr int S = amph_ctx::kSlots;
  static_assert(S >= 3, "one stream per engine");
  HIP_TRY(use_device(c->device));
  for (int s = 0; s < S; ++s) {
    if (!c->streams[s]) HIP_TRY(hipStreamCreateWithFlags(&c->streams[s], hipStreamNonBlocking));
    amph_ctx::Slot& sl = c->slots[s];
    for (hipEvent_t* e : {&sl.in_done, &sl.k_done, &sl.out_done})
      if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    sl.busy = false;
    sl.used = false;
  }
  hipStream_t s_in = c->streams[0], s_k = c->streams[1], s_out = c->streams[2];
  if (!c->pool) c->pool.reset(new amph::CopyPool(host_threads() - 1));
  size_t bpw = 0;
  for (const WordArrays* v : {&ins, &outs})
    for (const WordArray& x : *v) bpw += x.bytes_per_word;
  const size_t bw = batch_for(c, words, bpw);
  const size_t nb = (words + bw - 1) / bw;
  std::vector<char> in_pinned(ins.size()), out_pinned(outs.size());
  size_t dev_bytes = 0, hin_bytes = 0, hout_bytes = 0;
  // which arrays are DMA'd in place, and the slot bytes the others are staged through
  auto plan = [&](const WordArrays& v, std::vector<char>& pinned, size_t& staged) {
    for (size_t k = 0; k < v.size(); ++k) {
      pinned[k] = !v[k].io && amph::is_pinned_host(v[k].host);
      dev_bytes += align256(bw * v[k].bytes_per_word);
      if (!pinned[k]) staged += align256(bw * v[k].bytes_per_word);
    }
  };
  plan(ins, in_pinned, hin_bytes);
  plan(outs, out_pinned, hout_bytes);
  for (int s = 0; s < S && (size_t)s < nb; ++s) {
    hipError_t e = dev_ensure(c, c->slots[s].dev, dev_bytes);
    if (e == hipSuccess) e = c->slots[s].hin.ensure(hin_bytes);
    if (e == hipSuccess) e = c->slots[s].hout.ensure(hout_bytes);
    if (e != hipSuccess) return fail(AMPH_E_NOMEM, std::string("batch buffers: ") + hipGetErrorString(e));
  }
  if (with_ff) {
    hipError_t e = dev_ensure(c, c->ff, nb * sizeof(unsigned long long));
    if (e != hipSuccess) return fail(AMPH_E_NOMEM, "first-fail words");
    HIP_TRY(hipMemsetAsync(c->ff.p, 0x7F, nb * sizeof(unsigned long long), s_k));
  }
  // copy a finished batch's pageable outputs from the slot's staging buffer
  auto drain_out = [&](amph_ctx::Slot& sl) -> int {
    if (!sl.busy) return AMPH_OK;
    HIP_TRY(hipEventSynchronize(sl.out_done));
    std::vector<amph::CopyTask> tasks;
    size_t off = 0;
    for (size_t k = 0; k < outs.size(); ++k) {
      if (out_pinned[k]) continue;
      tasks.push_back(copy_out(outs[k], sl.base, sl.cnt, (char*)sl.hout.p + off));
      off += align256(bw * outs[k].bytes_per_word);
    }
    const int cst = c->pool->copy(tasks);
    sl.busy = false;
    return cst ? io_failed() : AMPH_OK;
  };
  for (size_t b = 0; b < nb; ++b) {
    amph_ctx::Slot& sl = c->slots[b % S];
    const size_t base = b * bw, cnt = std::min(bw, words - base);
    // stage pageable inputs into the slot's page-locked buffer once the slot's
    // previous HtoD has read it
    std::vector<amph::CopyTask> tasks;
    std::vector<const void*> src(ins.size());
    size_t hoff = 0;
    for (size_t k = 0; k < ins.size(); ++k) {
      if (in_pinned[k]) {
        src[k] = ins[k].host + (ins[k].base + base) * ins[k].bytes_per_word;
      } else {
        void* d = (char*)sl.hin.p + hoff;
        tasks.push_back(copy_in(ins[k], base, cnt, d));
        src[k] = d;
        hoff += align256(bw * ins[k].bytes_per_word);
      }
    }
    if (!tasks.empty()) {
      if (sl.used) HIP_TRY(hipEventSynchronize(sl.in_done));
      if (c->pool->copy(tasks)) return io_failed();
    }
    uint8_t* cur = (uint8_t*)sl.dev.p;
    std::vector<const uint4*> din;
    std::vector<uint4*> dout;
    if (sl.used) HIP_TRY(hipStreamWaitEvent(s_in, sl.k_done, 0));  // inputs consumed
    for (size_t k = 0; k < ins.size(); ++k) {
      HIP_TRY(hipMemcpyAsync(cur, src[k], cnt * ins[k].bytes_per_word, hipMemcpyHostToDevice, s_in));
      din.push_back((const uint4*)cur);
      cur += align256(bw * ins[k].bytes_per_word);
    }
    HIP_TRY(hipEventRecord(sl.in_done, s_in));
    for (size_t k = 0; k < outs.size(); ++k) {
      dout.push_back((uint4*)cur);
      cur += align256(bw * outs[k].bytes_per_word);
    }
    HIP_TRY(hipStreamWaitEvent(s_k, sl.in_done, 0));
    if (sl.used) HIP_TRY(hipStreamWaitEvent(s_k, sl.out_done, 0));  // outputs copied out
    unsigned long long* ff = with_ff ? (unsigned long long*)c->ff.p + b : nullptr;
    amph::LaunchCfg lc = cfg(c, s_k, cnt);
    lc.base = base;
    hipError_t e = launch(din, dout, cnt, ff, lc);
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    HIP_TRY(hipEventRecord(sl.k_done, s_k));
    // the slot's staging buffer still holds the previous batch's outputs
    if (int rc = drain_out(sl)) return rc;
    HIP_TRY(hipStreamWaitEvent(s_out, sl.k_done, 0));
    size_t ooff = 0;
    for (size_t k = 0; k < outs.size(); ++k) {
      void* dst = outs[k].host + (outs[k].base + base) * outs[k].bytes_per_word;
      if (!out_pinned[k]) {
        dst = (char*)sl.hout.p + ooff;
        ooff += align256(bw * outs[k].bytes_per_word);
      }
      HIP_TRY(hipMemcpyAsync(dst, dout[k], cnt * outs[k].bytes_per_word, hipMemcpyDeviceToHost, s_out));
    }
    HIP_TRY(hipEventRecord(sl.out_done, s_out));
    sl.busy = hout_bytes > 0;  // page-locked outputs need no copy-out (s_out is synced below)
    sl.used = true;
    sl.base = base;
    sl.cnt = cnt;
  }
  for (size_t b = nb > (size_t)S ? nb - S : 0; b < nb; ++b)
    if (int rc = drain_out(c->slots[b % S])) return rc;
  HIP_TRY(hipStreamSynchronize(s_out));  // page-locked outputs (no staging slot) landed too
  // a call with no outputs (amph_verify, the verify-only tail of
  // amph_mask_input) has nothing on s_out that waits for its kernels: wait
  // for them before the verdicts are read (the blocking copy below runs on
  // the null stream, which does not order with non-blocking streams)
  HIP_TRY(hipStreamSynchronize(s_k));
  if (with_ff) {
    std::vector<unsigned long long> h(nb);
    HIP_TRY(hipMemcpy(h.data(), c->ff.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < nb; ++b) {
      if (h[b] != amph::kNoFail) {
        if (first_fail) *first_fail = (int64_t)(b * bw * ff_scale + h[b]);
        return AMPH_E_VERIFY;
      }
    }
  }
  return AMPH_OK;
}

}  // namespace

// ---- small host calls ------------------------------------------------------------
// A host call whose inputs and outputs together fit c->small_bytes (default
// 2 MiB; AMPH_SMALL_BYTES, 0 = off) skips the batched pipeline: the inputs
// are memcpy'd into the context's page-locked arena, the kernel reads them
// and writes its outputs there in place (hipHostMalloc memory is mapped into
// the device's address space), its verdict words go from device memory to
// the arena by one 64-lane copy kernel, and the call makes ONE stream
// synchronisation -- no DMA round trips, events or staging threads.  At C1
// sizes (1 k words) each host call is then launch + PCIe latency, where the
// batched path paid three streams' worth of copies and synchronisations.
// Kernel stores to the arena are visible to the host once the stream has
// synchronised (end-of-kernel system-scope release); the CPU's memcpy into
// it completes before the launch is issued.

// the context's own stream k (host mode), created on first use
int host_stream(amph_ctx* c, int k, hipStream_t* s) {
  if (!c->streams[k]) HIP_TRY(hipStreamCreateWithFlags(&c->streams[k], hipStreamNonBlocking));
  *s = c->streams[k];
  return AMPH_OK;
}

bool small_call(const amph_ctx* c, size_t bytes) { return c->small_bytes && bytes <= c->small_bytes; }

// device bytes of arrays carved by Stager::take
size_t carve_bytes(std::initializer_list<size_t> sizes) {
  size_t t = 0;
  for (size_t b : sizes) t += align256(b ? b : 16);
  return t;
}

int Stager::begin(amph_ctx* ctx, hipStream_t stream, bool use_small, size_t bytes, int verdict_words, DevBuf* dev,
                  size_t dev_bytes, const char* what) {
  c = ctx, s = stream, small = use_small, n_ff = verdict_words;
  if (small) {
    if (c->small.ensure(bytes + 256) != hipSuccess) return fail(AMPH_E_NOMEM, "small-call arena");
    if (dev_ensure(c, c->small_ff, 256) != hipSuccess) return fail(AMPH_E_NOMEM, "small-call verdict words");
    if (c->small_ff_dirty) {  // an earlier call left them unknown
      HIP_TRY(hipMemsetAsync(c->small_ff.p, 0x7F, 256, s));
      c->small_ff_dirty = false;
    }
    base = (uint8_t*)c->small.p;
    off = 256;
    fl = (unsigned long long*)c->small_ff.p;
  }
  if (dev_bytes) {
    if (dev_ensure(c, *dev, dev_bytes) != hipSuccess) return fail(AMPH_E_NOMEM, what);
    dev_base = (uint8_t*)dev->p;
  }
  if (!small) base = dev_base;
  return AMPH_OK;
}
unsigned long long* Stager::result_word() {
  return small ? (unsigned long long*)c->small.p : (unsigned long long*)take(8);
}
hipError_t Stager::put(void* dst, const void* src, size_t bytes) {
  if (small) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
  }
  return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}
int Stager::arm() {
  if (small || !n_ff) return AMPH_OK;
  fl = (unsigned long long*)take(8 * n_ff);
  HIP_TRY(hipMemsetAsync(fl, 0x7F, 8 * n_ff, s));
  return AMPH_OK;
}
int Stager::finish(int64_t* v, std::initializer_list<ReadBack> outs) {
  if (!small) {
    HIP_TRY(read_back(s, {{v, fl, 8 * (size_t)n_ff}}));
    for (const ReadBack& r : outs)
      if (r.bytes) HIP_TRY(hipMemcpy(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost));
    return AMPH_OK;
  }
  hipError_t e = amph::launch_take_words(fl, (unsigned long long*)c->small.p, n_ff, s);
  if (e != hipSuccess) return launch_failed(e, "verdict copy");
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    c->small_ff_dirty = true;
    return hip_fail(e, "small-call synchronise");
  }
  if (n_ff) std::memcpy(v, c->small.p, 8 * (size_t)n_ff);
  return fetch(outs);
}
int Stager::fetch(std::initializer_list<ReadBack> outs) {
  if (!small) {
    HIP_TRY(read_back(s, outs));
    return AMPH_OK;
  }
  for (const ReadBack& r : outs)
    if (r.bytes) std::memcpy(r.dst, r.src, r.bytes);
  return AMPH_OK;
}
int Stager::launch_failed(hipError_t e, const char* what) {
  if (small) {
    c->small_ff_dirty = true;
    (void)hipStreamSynchronize(s);
  }
  return hip_fail(e, what);
}

namespace {
int run_small(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
              int64_t* first_fail, const Launch& launch, size_t bytes) {
  if (first_fail) *first_fail = -1;
  if (words == 0) return AMPH_OK;
  HIP_TRY(use_device(c->device));
  hipStream_t s;
  if (int st = host_stream(c, 1, &s)) return st;
  Stager h;
  if (int st = h.begin(c, s, true, bytes, with_ff ? 1 : 0)) return st;
  DevIn din;
  DevOut dout;
  for (const WordArray& x : ins) {
    uint8_t* p = h.take(words * x.bytes_per_word);
    if (amph::run_copy(copy_in(x, 0, words, p))) return io_failed();
    din.push_back((const uint4*)p);
  }
  for (const WordArray& x : outs) dout.push_back((uint4*)h.take(words * x.bytes_per_word));
  hipError_t e = launch(din, dout, words, with_ff ? h.fl : nullptr, cfg(c, s, words));
  if (e != hipSuccess) return h.launch_failed(e, "kernel launch");
  int64_t v = (int64_t)amph::kNoFail;
  if (int st = h.finish(&v, {})) return st;
  for (size_t k = 0; k < outs.size(); ++k)
    if (amph::run_copy(copy_out(outs[k], 0, words, dout[k]))) return io_failed();
  if (v != (int64_t)amph::kNoFail) {
    if (first_fail) *first_fail = v;
    return AMPH_E_VERIFY;
  }
  return AMPH_OK;
}

size_t call_bytes(size_t words, const WordArrays& ins, const WordArrays& outs) {
  size_t b = 0;
  for (const WordArrays* v : {&ins, &outs})
    for (const WordArray& x : *v) b += align256(words * x.bytes_per_word);
  return b;
}

}  // namespace

// An error part-way through leaves earlier batches' copies in flight (into
// the caller's page-locked buffers, or the slots): wait for them before
// returning, so nothing writes caller memory after the call has returned.
namespace {
int run_pipeline(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
                 int64_t* first_fail, const Launch& launch, size_t ff_scale) {
  const int rc = run_batched_impl(c, words, ins, outs, with_ff, first_fail, launch, ff_scale);
  if (rc != AMPH_OK && rc != AMPH_E_VERIFY) {
    for (int s = 0; s < amph_ctx::kSlots; ++s) {
      if (c->streams[s]) (void)hipStreamSynchronize(c->streams[s]);
      c->slots[s].busy = false;
    }
  }
  return rc;
}
}  // namespace

int run_batched(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
                int64_t* first_fail, const Launch& launch, size_t ff_scale) {
  if (g_host_io) {  // the entry point's AMPH_F_HOST_IO: the pointers are descriptors
    WordArrays ins2(ins), outs2(outs);
    for (WordArrays* v : {&ins2, &outs2})
      for (WordArray& x : *v) {
        x.io = (const amph_host_array*)x.host;
        if (words && (!x.io || !(x.out ? (bool)x.io->write : (bool)x.io->read)))
          return fail(AMPH_E_PARAM, x.out ? "host array without a write callback"
                                          : "host array without a read callback");
      }
    g_host_io = false;  // consumed: the nested call sees explicit descriptors
    const int st = run_batched(c, words, ins2, outs2, with_ff, first_fail, launch, ff_scale);
    g_host_io = true;
    return st;
  }
  if (!c->sub.empty()) return run_sharded(c, words, ins, outs, with_ff, first_fail, launch, ff_scale);
  const size_t bytes = call_bytes(words, ins, outs);
  if (small_call(c, bytes)) return run_small(c, words, ins, outs, with_ff, first_fail, launch, bytes);
  return run_pipeline(c, words, ins, outs, with_ff, first_fail, launch, ff_scale);
}

// ---- packed calls ----------------------------------------------------------------
// The verdicts of a packed call live in a device array of one word per object
// (c->seg, after the offsets table) that every batch's kernel min-combines
// into; the pipeline's own per-batch first-fail words are not used.
namespace {
// the verdict array as the caller's first_fail entries and the call's status
int packed_status(const unsigned long long* v, size_t n_objects, int64_t* first_fail) {
  size_t failed = 0, first = 0;
  for (size_t o = 0; o < n_objects; ++o) {
    const bool bad = v[o] != amph::kNoFail;
    if (bad && !failed++) first = o;
    if (first_fail) first_fail[o] = bad ? (int64_t)v[o] : -1;
  }
  if (!failed) return AMPH_OK;
  return fail(AMPH_E_VERIFY, "Verification of secret has failed: object " + std::to_string(first) + " at word " +
                                 std::to_string(v[first]) + " (" + std::to_string(failed) + " of " +
                                 std::to_string(n_objects) + " objects failed)");
}

// run_small for a packed call: the table sits in the arena too (only a
// failing lane reads it), the verdict array in device memory (atomics) and
// comes to the arena by a copy kernel before the call's ONE synchronisation.
int run_packed_small(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs,
                     const uint64_t* offsets, size_t n_objects, int64_t* first_fail, const SegLaunch& launch,
                     size_t bytes) {
  hipStream_t s;
  if (int st = host_stream(c, 1, &s)) return st;
  Stager h;
  if (int st = h.begin(c, s, true, bytes, 0, &c->seg, align256(8 * n_objects), "verdict array")) return st;
  DevIn din;
  DevOut dout;
  for (const WordArray& x : ins) {
    uint8_t* p = h.take(words * x.bytes_per_word);
    if (amph::run_copy(copy_in(x, 0, words, p))) return io_failed();
    din.push_back((const uint4*)p);
  }
  for (const WordArray& x : outs) dout.push_back((uint4*)h.take(words * x.bytes_per_word));
  uint64_t* tab = (uint64_t*)h.take(8 * (n_objects + 1));
  std::memcpy(tab, offsets, 8 * (n_objects + 1));
  unsigned long long* hv = (unsigned long long*)h.take(8 * n_objects);
  unsigned long long* dv = (unsigned long long*)c->seg.p;
  HIP_TRY(hipMemsetAsync(dv, 0x7F, 8 * n_objects, s));
  hipError_t e = launch(din, dout, words, 0, tab, dv, cfg(c, s, words));
  if (e != hipSuccess) return h.launch_failed(e, "kernel launch");
  e = amph::launch_take_array(dv, hv, n_objects, s);
  if (e != hipSuccess) return h.launch_failed(e, "verdict copy");
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "small-call synchronise");
  for (size_t k = 0; k < outs.size(); ++k)
    if (amph::run_copy(copy_out(outs[k], 0, words, dout[k]))) return io_failed();
  return packed_status(hv, n_objects, first_fail);
}
}  // namespace

int run_packed(amph_ctx* c, size_t words, const WordArrays& ins, const WordArrays& outs, const uint64_t* offsets,
               size_t n_objects, int64_t* first_fail, const SegLaunch& launch) {
  if (n_objects == 0) return AMPH_OK;
  if (words == 0) {  // nothing to verify: every object reads "verified"
    for (size_t o = 0; first_fail && o < n_objects; ++o) first_fail[o] = -1;
    return AMPH_OK;
  }
  HIP_TRY(use_device(c->device));
  const size_t tab_bytes = align256(8 * (n_objects + 1)), ff_bytes = align256(8 * n_objects);
  const size_t bytes = call_bytes(words, ins, outs) + tab_bytes + ff_bytes;
  if (small_call(c, bytes)) return run_packed_small(c, words, ins, outs, offsets, n_objects, first_fail, launch, bytes);
  hipStream_t s_k;
  if (int st = host_stream(c, 1, &s_k)) return st;
  if (dev_ensure(c, c->seg, tab_bytes + ff_bytes) != hipSuccess) return fail(AMPH_E_NOMEM, "offsets table");
  const uint64_t* tab = (const uint64_t*)c->seg.p;
  unsigned long long* dv = (unsigned long long*)((uint8_t*)c->seg.p + tab_bytes);
  // kPageableRule: the context's streams are idle between calls
  HIP_TRY(hipMemcpy(c->seg.p, offsets, 8 * (n_objects + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(dv, 0x7F, 8 * n_objects, s_k));
  auto batch = [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                   const amph::LaunchCfg& lc) { return launch(din, dout, cnt, lc.base, tab, dv, lc); };
  if (int st = run_pipeline(c, words, ins, outs, false, nullptr, batch, 1)) return st;
  std::vector<unsigned long long> v(n_objects);  // the pipeline has synchronised the kernel stream
  HIP_TRY(hipMemcpy(v.data(), dv, 8 * n_objects, hipMemcpyDeviceToHost));
  return packed_status(v.data(), n_objects, first_fail);
}

// Multi-device context: contiguous shards of ceil(words / ndev), one thread
// per device running that device's own batched pipeline; the first failing
// shard (in word order) gives the global first-fail index.
namespace {
int run_sharded(amph_ctx* g, size_t words, const WordArrays& ins, const WordArrays& outs, bool with_ff,
                int64_t* first_fail, const Launch& launch, size_t ff_scale) {
  if (first_fail) *first_fail = -1;
  drop_launch_timing();  // per-launch timing is single-device only
  if (words == 0) return AMPH_OK;
  const size_t nd = g->sub.size(), per = (words + nd - 1) / nd;
  struct Res {
    int st = AMPH_OK;
    int64_t ff = -1;
    std::string err;
  };
  std::vector<Res> res(nd);
  size_t used = 0;
  while (used < nd && used * per < words) ++used;
  amph::Latch done(used);
  for (size_t d = 0; d < used; ++d) {
    const size_t start = d * per, cnt = std::min(per, words - start);
    WordArrays in2(ins), out2(outs);
    for (WordArrays* v : {&in2, &out2})
      for (WordArray& x : *v) x.base += start;
    amph_ctx* s = g->sub[d];
    s->worker->post([&, d, s, cnt, in2 = std::move(in2), out2 = std::move(out2)]() {
      try {
        std::lock_guard<std::mutex> lk(s->mu);
        res[d].st = run_batched(s, cnt, in2, out2, with_ff, &res[d].ff, launch, ff_scale);
      } catch (const std::exception& e) {
        res[d].st = fail(AMPH_E_NOMEM, e.what());
      }
      if (res[d].st != AMPH_OK) res[d].err = last_error();
      s->worker_tasks.fetch_add(1, std::memory_order_relaxed);
      done.count_down();
    });
  }
  done.wait();
  for (size_t d = 0; d < used; ++d)
    if (res[d].st != AMPH_OK && res[d].st != AMPH_E_VERIFY) return fail(res[d].st, res[d].err);
  for (size_t d = 0; d < used; ++d)
    if (res[d].st == AMPH_E_VERIFY) {
      if (first_fail) *first_fail = (int64_t)(d * per * ff_scale) + res[d].ff;
      return AMPH_E_VERIFY;
    }
  return AMPH_OK;
}

}  // namespace

int check_dev_words(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p && ((uintptr_t)p & 15))
      return fail(AMPH_E_PARAM, "device word arrays must be 16-byte aligned");
  return AMPH_OK;
}

// 24-character base64 records move as 8-byte vectors
int check_dev_records(const void* p) {
  if (p && ((uintptr_t)p & 7))
    return fail(AMPH_E_PARAM, "device base64 record arrays must be 8-byte aligned");
  return AMPH_OK;
}

int reset_ff_dev(int64_t* ff, uint32_t flags, hipStream_t s) {
  if (!ff) return fail(AMPH_E_PARAM, "first_fail is required");
  if ((uintptr_t)ff & 7) return fail(AMPH_E_PARAM, "first_fail must be 8-byte aligned");
  if (!(flags & AMPH_F_ACCUMULATE)) HIP_TRY(hipMemsetAsync(ff, 0x7F, sizeof(int64_t), s));
  return AMPH_OK;
}

int run_words(amph_ctx* c, size_t words, const WordArrays& arrays, bool with_ff, int64_t* first_fail,
              uint32_t flags, void* stream, const char* kernel, const Launch& launch) {
  const bool dev = flags & AMPH_F_DEVICE;
  WordArrays ins, outs;
  DevIn din;
  DevOut dout;
  for (const WordArray& x : arrays) {
    if (dev && x.dev_align == 16)
      if (int st = check_dev_words({x.host})) return st;
    if (dev && x.dev_align == 8)
      if (int st = check_dev_records(x.host)) return st;
    (x.out ? outs : ins).push_back(x);
    if (x.out) dout.push_back((uint4*)x.host);
    else din.push_back((const uint4*)x.host);
  }
  if (dev) {
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(use_device(c->device));
    if (with_ff)
      if (int st = reset_ff_dev(first_fail, flags, s)) return st;
    hipError_t e = launch(din, dout, words, (unsigned long long*)first_fail, cfg(c, s, words));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, kernel);
  }
  std::lock_guard<std::mutex> g(c->mu);
  return run_batched(c, words, ins, outs, with_ff, first_fail, launch);
}
}  // namespace capi
