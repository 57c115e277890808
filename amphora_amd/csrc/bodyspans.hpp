// Where the five base64 members lie inside a response body, and which aligned
// 16-byte granules hold a text that starts at any byte (include/
// amphora_client_bodies.h).  Shared by the host calls (amph_bodies_*), the
// any-alignment form of k_acc_b64 (wire.hip) and the CPU tests, so it compiles
// for the host alone (as wiretiles.hpp and seglookup.hpp) and includes no HIP
// header.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "seglookup.hpp"

namespace amph {

// ---- the scanner ---------------------------------------------------------------
// One VerifiableSecretShare / OutputDeliveryObject JSON body -> byte start and
// length of the five top-level members' values in ODO order (secretShares,
// rShares, vShares, wShares, uShares), the quotes excluded.  Only structure is
// walked, as wire._top_level_members does: strings are skipped whole with
// their backslash escapes counted, the nesting depth is tracked, and a key
// deeper than depth 1 -- a tag whose key or value is "rShares" -- is no member.
// Anything but the plain form is refused with its reason; wire.odo_field_texts
// stays the one place that defines what happens then.  Nothing outside
// [body, body + len) is read.
enum BodyScan {
  kBodyOk = 0,
  kBodyNoObject,      // the first structural character is not '{'
  kBodyMissing,       // a member is missing
  kBodyNotString,     // a member's value is null or no string
  kBodyTwice,         // a member is given twice
  kBodyEscape,        // a backslash inside a member's value
  kBodyUnterminated,  // a string without its closing quote
};

inline const char* body_scan_reason(int r) {
  static const char* const kWhat[] = {"plain",
                                      "no enclosing object",
                                      "a member is missing",
                                      "a member is null or not a string",
                                      "a member is given twice",
                                      "a backslash inside a member's value",
                                      "an unterminated string"};
  return r >= 0 && r <= kBodyUnterminated ? kWhat[r] : "?";
}

namespace bodyspans_detail {
constexpr const char* kNames[5] = {"secretShares", "rShares", "vShares", "wShares", "uShares"};
inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
// the index of the quote that closes the string opening at body[i] ('"'), or
// len: every backslash takes the byte after it along
inline size_t string_end(const char* body, size_t len, size_t i) {
  for (size_t k = i + 1; k < len; ++k) {
    if (body[k] == '\\') ++k;
    else if (body[k] == '"') return k;
  }
  return len;
}
}  // namespace bodyspans_detail

inline BodyScan body_scan(const char* body, size_t len, uint64_t starts[5], uint64_t lens[5]) {
  using namespace bodyspans_detail;
  bool have[5] = {false, false, false, false, false};
  size_t depth = 0, pos = 0;
  bool opened = false;
  while (pos < len) {
    const char c = body[pos];
    if (c == '"') {
      const size_t e = string_end(body, len, pos);
      if (e >= len) return kBodyUnterminated;
      size_t next = e + 1;
      if (depth == 1) {
        size_t j = e + 1;
        while (j < len && is_space(body[j])) ++j;
        if (j < len && body[j] == ':') {  // a key of the outermost object
          const size_t klen = e - pos - 1;
          for (int k = 0; k < 5; ++k) {
            if (klen != strlen(kNames[k]) || memcmp(body + pos + 1, kNames[k], klen) != 0) continue;
            if (have[k]) return kBodyTwice;
            size_t v = j + 1;
            while (v < len && is_space(body[v])) ++v;
            if (v >= len || body[v] != '"') return kBodyNotString;
            const char* first = body + v + 1;
            const char* q = (const char*)memchr(first, '"', len - (v + 1));
            if (!q) return kBodyUnterminated;
            // (a backslash before the first quote: the value is no plain base64 text)
            if (memchr(first, '\\', (size_t)(q - first))) return kBodyEscape;
            have[k] = true;
            starts[k] = v + 1;
            lens[k] = (uint64_t)(q - first);
            next = (size_t)(q - body) + 1;
            break;
          }
        }
      }
      pos = next;
      continue;
    }
    if (c == '{' || c == '[') {
      if (!opened && c != '{') return kBodyNoObject;
      opened = true;
      ++depth;
    } else if (c == '}' || c == ']') {
      if (depth == 0) return kBodyNoObject;
      if (--depth == 0) break;  // the outermost object is closed: what follows is not looked at
    }
    ++pos;
  }
  if (!opened) return kBodyNoObject;
  for (int k = 0; k < 5; ++k)
    if (!have[k]) return kBodyMissing;
  return kBodyOk;
}

// ---- the granule rule ----------------------------------------------------------
// A text of nchars characters at byte `start` of a 16-byte aligned buffer;
// granule g is bytes [16 g, 16 g + 16).  The kernel loads whole granules and
// funnels a unit's 16 characters out of one or two of them; it loads a granule
// only if the rule names it, and the rule names only granules that hold at
// least one character of the text.
struct BodyGranules {
  uint64_t first, end;  // half-open; first == end for an empty text
};
AMPH_SEG_HD inline BodyGranules body_granules(uint64_t start, uint64_t nchars) {
  if (nchars == 0) return BodyGranules{start >> 4, start >> 4};
  return BodyGranules{start >> 4, ((start + nchars - 1) >> 4) + 1};
}

// The granules of 16-character unit `unit` (characters [16 unit, 16 unit + 16)
// cut at nchars): `first`, and first + 1 when n == 2.  n == 0: the unit lies
// past the text.  residue: the byte of granule `first` where the unit starts
// (start & 15 for every unit of the text).
struct BodyUnit {
  uint64_t first;
  uint32_t n, residue;
};
AMPH_SEG_HD inline BodyUnit body_unit(uint64_t start, uint64_t nchars, uint64_t unit) {
  const uint64_t c0 = 16 * unit;
  if (c0 >= nchars) return BodyUnit{(start + c0) >> 4, 0u, (uint32_t)(start & 15)};
  const uint64_t c1 = c0 + 16 < nchars ? c0 + 16 : nchars;  // one past the unit's last character
  const uint64_t g0 = (start + c0) >> 4, g1 = (start + c1 - 1) >> 4;
  return BodyUnit{g0, (uint32_t)(g1 - g0) + 1u, (uint32_t)(start & 15)};
}

}  // namespace amph
