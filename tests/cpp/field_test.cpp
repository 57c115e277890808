// Host driver of amphora_amd/csrc/field.hpp for tests/test_field_host.py.
//
// Reads lines "op p a b [c d]" (hex, 128-bit) on stdin, fills an Fp for p the
// way capi_ctx.hip's setup_field does (n0 by Newton iteration, R^2 by 128
// modular doublings, big = p > 2^127) and prints one hex result per line:
//
//   cios  a b      mont_mul_cios(a, b)       a < 2^128, b < p
//   ps    a b      mont_mul_ps(a, b)         a < 2^128, b < p
//   redc  a        redc(a)                   a < 2^128
//   dot2  x y u v  dot2_redc(x, y, u, v)     x, u < p; y, v < 2^128
//   add   a b      mod_add(a, b)             a, b < p
//   sub   a b      mod_sub(a, b)             a, b < p
//   cant  a        canon<true>(a)            p > 2^127
//   canf  a        canon<false>(a)
//
// The host fallbacks of addc / subc / macc96 run here; the device builtins and
// the inline assembly are pinned by the GPU suite (tests/test_hip_primes.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "field.hpp"

typedef unsigned __int128 u128;
using amph::Fp;
using amph::W4;

static W4 w4_of(u128 x) {
  return W4{{(uint32_t)x, (uint32_t)(x >> 32), (uint32_t)(x >> 64), (uint32_t)(x >> 96)}};
}

static u128 u128_of(const W4& a) {
  return (u128)a.v[0] | ((u128)a.v[1] << 32) | ((u128)a.v[2] << 64) | ((u128)a.v[3] << 96);
}

static u128 add_mod(u128 a, u128 b, u128 p) {  // a, b < p
  u128 s = a + b;
  if (s < a || s >= p) s -= p;
  return s;
}

static Fp make_field(u128 p) {
  Fp f{};
  const W4 pw = w4_of(p);
  for (int i = 0; i < 4; ++i) f.p[i] = pw.v[i];
  uint32_t inv = f.p[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - f.p[0] * inv;
  f.n0 = (uint32_t)(0u - inv);
  u128 x = ((u128)0 - p) % p;
  for (int i = 0; i < 128; ++i) x = add_mod(x, x, p);
  const W4 r2 = w4_of(x);
  for (int i = 0; i < 4; ++i) f.r2[i] = r2.v[i];
  f.big = (p >> 127) != 0;
  return f;
}

static bool parse_hex(const char* s, u128* out) {
  u128 x = 0;
  int n = 0;
  for (; *s; ++s, ++n) {
    int d;
    if (*s >= '0' && *s <= '9') d = *s - '0';
    else if (*s >= 'a' && *s <= 'f') d = *s - 'a' + 10;
    else if (*s >= 'A' && *s <= 'F') d = *s - 'A' + 10;
    else return false;
    if (n >= 32) return false;
    x = (x << 4) | (u128)d;
  }
  *out = x;
  return n > 0;
}

static void print_hex(u128 x) {
  std::printf("%016llx%016llx\n", (unsigned long long)(x >> 64), (unsigned long long)x);
}

int main() {
  char line[512];
  u128 cur_p = 0;
  Fp f{};
  long lineno = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    ++lineno;
    char* tok[8];
    int nt = 0;
    for (char* t = std::strtok(line, " \t\r\n"); t && nt < 8; t = std::strtok(nullptr, " \t\r\n")) tok[nt++] = t;
    if (nt == 0) continue;
    u128 v[5] = {0, 0, 0, 0, 0};
    bool ok = nt >= 3 && nt <= 6;
    for (int i = 1; ok && i < nt; ++i) ok = parse_hex(tok[i], &v[i - 1]);
    const std::string op = tok[0];
    const int nargs = nt - 2;
    const int want = op == "dot2" ? 4 : (op == "redc" || op == "cant" || op == "canf") ? 1 : 2;
    if (!ok || nargs != want || v[0] < 3 || (v[0] & 1) == 0) {
      std::fprintf(stderr, "field_test: bad line %ld\n", lineno);
      return 2;
    }
    if (v[0] != cur_p) {
      cur_p = v[0];
      f = make_field(cur_p);
    }
    const W4 a = w4_of(v[1]), b = w4_of(v[2]), c = w4_of(v[3]), d = w4_of(v[4]);
    W4 r;
    if (op == "cios") r = amph::mont_mul_cios(a, b, f);
    else if (op == "ps") r = amph::mont_mul_ps(a, b, f);
    else if (op == "redc") r = amph::redc(a, f);
    else if (op == "dot2") r = amph::dot2_redc(a, b, c, d, f);
    else if (op == "add") r = amph::mod_add(a, b, f);
    else if (op == "sub") r = amph::mod_sub(a, b, f);
    else if (op == "cant") r = amph::canon<true>(a, f);
    else if (op == "canf") r = amph::canon<false>(a, f);
    else {
      std::fprintf(stderr, "field_test: unknown op at line %ld\n", lineno);
      return 2;
    }
    print_hex(u128_of(r));
  }
  return 0;
}
