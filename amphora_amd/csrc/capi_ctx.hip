// C ABI of libamphora_hip (declared in include/amphora.h): the last error,
// timing events, field setup, context lifetime and statistics, host-memory
// registration.
#include "capi_internal.hpp"

namespace capi __attribute__((visibility("hidden"))) {
namespace {
thread_local std::string g_last_error;
thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;  // amph_time_next_launch
}  // namespace

const std::string& last_error() { return g_last_error; }
void drop_launch_timing() { g_ev_start = g_ev_stop = nullptr; }

int fail(int status, const std::string& msg) {
  g_last_error = msg;
  return status;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(AMPH_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

hipError_t use_device(int device) {
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur == device) return hipSuccess;
  return hipSetDevice(device);
}

// ---- device memory ------------------------------------------------------------
// (c->mu held) the party-session buffers pooled for reuse are the only device
// memory a context keeps that nothing is using: every allocation of the
// context that runs out of memory frees them and tries once more, so the
// pool never causes the out-of-memory error it would then report.
size_t pool_bytes(const amph_ctx* c) {
  size_t t = 0;
  for (const DevBuf& b : c->party_pool) t += b.cap;
  return t;
}

void pool_reclaim(amph_ctx* c) {
  for (DevBuf& b : c->party_pool) b.release();
  c->party_pool.clear();
}

hipError_t dev_ensure(amph_ctx* c, DevBuf& b, size_t bytes) {
  hipError_t e = b.ensure(bytes);
  if (e == hipErrorOutOfMemory && !c->party_pool.empty()) {
    (void)hipGetLastError();
    pool_reclaim(c);
    e = b.ensure(bytes);
  }
  return e;
}

// ---- field setup (host) -----------------------------------------------------
u128 add_mod(u128 a, u128 b, u128 p) {  // a, b < p
  u128 s = a + b;
  if (s < a || s >= p) s -= p;
  return s;
}

int setup_field(amph_ctx* c, const uint8_t* p_le, const uint8_t* r_le, const uint8_t* rinv_le) {
  const u128 p = ld128(p_le), r = ld128(r_le), rinv = ld128(rinv_le);
  if (p < 3 || (p & 1) == 0) return fail(AMPH_E_PARAM, "prime must be odd and > 2");
  const u128 R = ((u128)0 - p) % p;  // 2^128 mod p
  if (r != R) return fail(AMPH_E_PARAM, "r must equal 2^128 mod prime (MP-SPDZ auxiliary modulus)");
  Fp f{};
  const W4 pw = w4_of(p);
  for (int i = 0; i < 4; ++i) f.p[i] = pw.v[i];
  uint32_t inv = f.p[0];  // Newton: inv = p^-1 mod 2^32
  for (int i = 0; i < 5; ++i) inv *= 2u - f.p[0] * inv;
  f.n0 = (uint32_t)(0u - inv);
  u128 x = R;  // R^2 mod p = R * 2^128 mod p by 128 doublings
  for (int i = 0; i < 128; ++i) x = add_mod(x, x, p);
  const W4 r2 = w4_of(x);
  for (int i = 0; i < 4; ++i) f.r2[i] = r2.v[i];
  f.big = (p >> 127) != 0;
  if (rinv >= p) return fail(AMPH_E_PARAM, "rInv must be reduced mod prime");
  // r * rInv == 1 (mod p): mont_mul(mont_mul(r, rInv), R^2) = r rInv
  const W4 t = amph::mont_mul(amph::mont_mul(w4_of(r), w4_of(rinv), f), r2, f);
  if (u128_of(t) != 1) return fail(AMPH_E_PARAM, "rInv must be the inverse of r mod prime");
  c->f = f;
  c->p = p;
  c->r = r;
  c->rinv = rinv;
  return AMPH_OK;
}

u128 mulmod_host(const amph_ctx* c, u128 a, u128 b) {  // a < p
  return u128_of(amph::mont_mul(amph::mont_mul(w4_of(a), w4_of(b), c->f), amph::r2_word(c->f), c->f));
}

// Workgroup size: 1024 threads (16 waves).  Measured through bench.py on
// MI355X (gpurun_out r01c sweep): 1024 beat 128/256/512 by 2-5 % at both
// 1 Mi words x 2 parties and 16 Mi words x 3 parties.  AMPH_BLOCK overrides.
int block_for(const amph_ctx* c, size_t words) {
  (void)words;
  return c->block > 0 ? c->block : 1024;
}

amph::LaunchCfg cfg(amph_ctx* c, hipStream_t s, size_t words) {
  c->launches.fetch_add(1, std::memory_order_relaxed);
  amph::LaunchCfg lc{s, c->grid_cap, block_for(c, words)};
  lc.ev_start = g_ev_start;  // consumed by this launch only
  lc.ev_stop = g_ev_stop;
  g_ev_start = g_ev_stop = nullptr;
  return lc;
}
}  // namespace capi

// ============================================================================
extern "C" {

int amph_time_next_launch(void* start_event, void* stop_event) {
  g_ev_start = (hipEvent_t)start_event;
  g_ev_stop = (hipEvent_t)stop_event;
  return AMPH_OK;
}

int amph_timing_event_create(void** event) {
  if (!event) return fail(AMPH_E_PARAM, "null event");
  hipEvent_t e = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  *event = (void*)e;
  return AMPH_OK;
}

int amph_timing_event_destroy(void* event) {
  if (event) HIP_TRY(hipEventDestroy((hipEvent_t)event));
  return AMPH_OK;
}

int amph_timing_event_record(void* event, void* stream) {
  if (!event) return fail(AMPH_E_PARAM, "null event");
  HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
  return AMPH_OK;
}

int amph_timing_event_elapsed_ms(void* start_event, void* stop_event, float* ms) {
  if (!start_event || !stop_event || !ms) return fail(AMPH_E_PARAM, "null event or result");
  HIP_TRY(hipEventSynchronize((hipEvent_t)stop_event));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start_event, (hipEvent_t)stop_event));
  return AMPH_OK;
}

const char* amph_version(void) { return "amphora_amd 0.1.0 (gfx950)"; }

const char* amph_last_error(void) { return g_last_error.c_str(); }

const char* amph_strerror(int status) {
  switch (status) {
    case AMPH_OK: return "ok";
    case AMPH_E_VERIFY: return "Verification of secret has failed";
    case AMPH_E_LEN: return "length invariant violated";
    case AMPH_E_PARAM: return "invalid argument";
    case AMPH_E_HIP: return "HIP runtime error";
    case AMPH_E_NOMEM: return "out of memory";
    case AMPH_E_RANGE: return "array index out of range";
    default: return "unknown status";
  }
}

int amph_ctx_create(const uint8_t p_le[16], const uint8_t r_le[16], const uint8_t rinv_le[16],
                    int device, amph_ctx** out) {
  if (!out || !p_le || !r_le || !rinv_le) return fail(AMPH_E_PARAM, "null argument");
  *out = nullptr;
  amph_ctx* c = new (std::nothrow) amph_ctx();
  if (!c) return fail(AMPH_E_NOMEM, "context");
  int st = setup_field(c, p_le, r_le, rinv_le);
  if (st != AMPH_OK) {
    delete c;
    return st;
  }
  c->device = device;
  c->small.flags = hipHostMallocCoherent;  // kernels read and write the arena in place
  if (const char* g = std::getenv("AMPH_GRID_CAP")) c->grid_cap = std::max(0, std::atoi(g));
  if (const char* sb = std::getenv("AMPH_SMALL_BYTES")) c->small_bytes = (size_t)std::strtoull(sb, nullptr, 10);
  if (const char* pb = std::getenv("AMPH_PARTY_POOL_BYTES")) c->pool_cap_bytes = (size_t)std::strtoull(pb, nullptr, 10);
  if (const char* b = std::getenv("AMPH_BLOCK")) {
    const int v = std::atoi(b);
    if (v >= 64 && v <= amph::kMaxBlock && v % 64 == 0) c->block = v;
  }
  *out = c;
  return AMPH_OK;
}

int amph_ctx_create_multi(const uint8_t p_le[16], const uint8_t r_le[16],
                          const uint8_t rinv_le[16], const int* devices, int ndev,
                          amph_ctx** out) {
  if (!out || !devices || ndev < 1) return fail(AMPH_E_PARAM, "devices must name at least one device");
  if (ndev == 1) return amph_ctx_create(p_le, r_le, rinv_le, devices[0], out);
  *out = nullptr;
  amph_ctx* g = nullptr;
  if (int st = amph_ctx_create(p_le, r_le, rinv_le, devices[0], &g)) return st;
  for (int d = 0; d < ndev; ++d) {
    amph_ctx* s = nullptr;
    if (int st = amph_ctx_create(p_le, r_le, rinv_le, devices[d], &s)) {
      amph_ctx_destroy(g);
      return st;
    }
    s->worker.reset(new (std::nothrow) amph::DeviceWorker());
    g->sub.push_back(s);
    if (!s->worker) {
      amph_ctx_destroy(g);
      return fail(AMPH_E_NOMEM, "device worker thread");
    }
  }
  *out = g;
  return AMPH_OK;
}

int amph_ctx_device_count(const amph_ctx* c) {
  return c ? (c->sub.empty() ? 1 : (int)c->sub.size()) : 0;
}

void amph_ctx_destroy(amph_ctx* c) {
  if (!c) return;
  c->worker.reset();  // drains its queue and joins: nothing of c runs after this
  for (amph_ctx* s : c->sub) amph_ctx_destroy(s);
  c->sub.clear();
  if (c->streams[0] || c->slots[0].dev.p || c->ff.p) {
    (void)use_device(c->device);
    for (int s = 0; s < amph_ctx::kSlots; ++s) {
      if (c->streams[s]) (void)hipStreamSynchronize(c->streams[s]);
      c->slots[s].dev.release();
      c->slots[s].hin.release();
      c->slots[s].hout.release();
      for (hipEvent_t e : {c->slots[s].in_done, c->slots[s].k_done, c->slots[s].out_done})
        if (e) (void)hipEventDestroy(e);
      if (c->streams[s]) (void)hipStreamDestroy(c->streams[s]);
    }
    c->ff.release();
    c->tail.release();
    c->wire.release();
    c->wire_img.release();
    c->xstage.release();
  }
  if (c->small.p || c->small_ff.p) {
    (void)use_device(c->device);
    if (c->streams[1]) (void)hipStreamSynchronize(c->streams[1]);
    c->small.release();
    c->small_ff.release();
  }
  if (c->xdev_done) {
    (void)use_device(c->device);
    (void)hipEventSynchronize(c->xdev_done);
    (void)hipEventDestroy(c->xdev_done);
  }
  c->xdev.release();
  if (c->seg.p) {
    (void)use_device(c->device);
    c->seg.release();
  }
  if (!c->party_pool.empty()) {
    (void)use_device(c->device);
    for (DevBuf& b : c->party_pool) b.release();
  }
  delete c;
}

int amph_ctx_device(const amph_ctx* c) { return c ? c->device : -1; }

int amph_ctx_stats(amph_ctx* c, amph_stats* out) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (!out) return fail(AMPH_E_PARAM, "null stats output");
  *out = amph_stats{};
  auto add = [&](amph_ctx* x) {
    std::lock_guard<std::mutex> g(x->mu);
    out->kernel_launches += x->launches.load(std::memory_order_relaxed);
    out->pool_buffers += x->party_pool.size();
    out->pool_bytes += pool_bytes(x);
    out->device_workers += x->worker ? 1 : 0;
    out->worker_tasks += x->worker_tasks.load(std::memory_order_relaxed);
  };
  add(c);
  for (amph_ctx* s : c->sub) add(s);
  return AMPH_OK;
}

int amph_ctx_set_batch_words(amph_ctx* c, size_t words) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  std::lock_guard<std::mutex> g(c->mu);
  if (words) c->batch_words = words;
  for (amph_ctx* s : c->sub) amph_ctx_set_batch_words(s, words);
  return AMPH_OK;
}

int amph_host_register(amph_ctx* c, void* ptr, size_t bytes) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (!ptr || !bytes) return fail(AMPH_E_PARAM, "null or empty range");
  HIP_TRY(use_device(c->device));
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
  return AMPH_OK;
}

int amph_host_unregister(amph_ctx* c, void* ptr) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (!ptr) return fail(AMPH_E_PARAM, "null pointer");
  HIP_TRY(use_device(c->device));
  HIP_TRY(hipHostUnregister(ptr));
  return AMPH_OK;
}

}  // extern "C"
