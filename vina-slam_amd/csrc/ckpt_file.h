// ckpt_file.h — the checkpoint file's layout and its host-side validator
// (vg_checkpoint_save / vg_checkpoint_load, DESIGN.md §5 "Checkpoint").
// Host-only and free of HIP: tools/ckpt_check.cpp builds it into a stand-alone
// program for sanitizer runs over malformed files.
//
//   CkptHead | vg_config bytes | CkptSec[nsec] | pad to 16 | image
//
// The image is what the device packed: every section at a 16-byte aligned
// offset, its bytes the live prefix of one array (or the host mirror's blob),
// zero padding in between. Each section carries one 64-bit checksum over its
// little-endian 64-bit words (the last word zero-padded):
//   sum_i word[i] * (kCkptMul * (2 i + 1))   mod 2^64
// — a position-weighted sum, so it is order-independent to compute (a plain
// parallel reduction on the device, checkpoint.hip k_ckpt_sum) yet changes
// when two different words trade places. The head (with head_sum zeroed), the
// configuration and the table are covered by head_sum, same rule.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/vina_gpu.h"

namespace vg {

constexpr char kCkptMagic[8] = {'V', 'I', 'N', 'A', 'C', 'K', 'P', 'T'};
constexpr uint32_t kCkptVersion = 1;
constexpr uint64_t kCkptMul = 0x9E3779B97F4A7C15ull;
constexpr int kCkptMaxSec = 64;

// section ids; the record size of each (bytes per count) is ckpt_rec()
enum CkptId : uint32_t {
  kSecHdr = 1, kSecPlane, kSecPcrAdd, kSecPcrFix, kSecCovAdd, kSecEig, kSecJour, kSecDbox, kSecPcrs, kSecLseg,
  kSecInSlide, kSecSlide, kSecFixPnt, kSecFixVar, kSecWpPnt, kSecWpVar, kSecWpLeaf, kSecWpInt, kSecWpOrd,
  kSecSlots, kSecRootId, kSecRootKey, kSecDState, kSecHost, kSecEnd
};
constexpr int kCkptSlotInts = 32 + 32;     // slot_epoch[32], the map counters (padded to 32)
constexpr int kCkptDStateDoubles = 256 + 256 + 96 + 8 + 16 + 32 * 24 + 32 * 12 + 1 + 3 + 32 * (64 + 225) + 1;

struct CkptDims {
  int32_t n_nodes, n_fix, n_slide, n_roots;
  int32_t W, cap_wp, max_layer, pad;  // cap_wp: max_points_per_scan, the window arrays' slot stride (lseg run starts count from it)
  int32_t wpn[32];                    // window points per physical slot
  int32_t arena[32];                  // per slot: the wp_ord arena's cursor (0: never inserted)
  int32_t ord0[32];                   // per slot: wp_ord entries of the insert's leaf runs, packed from 0 (the
                                      // recut's follow from cap_wp up to the cursor)
};
struct CkptHead {
  char magic[8];
  uint32_t version, nsec, cfg_bytes, head_bytes;  // head_bytes: everything before the image
  uint64_t image_bytes, head_sum;
  CkptDims dims;
};
struct CkptSec {
  uint32_t id, rec;
  uint64_t off, bytes, count, sum;  // off: in the image
};
static_assert(sizeof(CkptHead) == 40 + 104 * 4, "CkptHead layout");
static_assert(sizeof(CkptSec) == 40, "CkptSec layout");

inline uint64_t ckpt_head_bytes(uint32_t nsec) {
  return (sizeof(CkptHead) + sizeof(vg_config) + (uint64_t)nsec * sizeof(CkptSec) + 15) & ~uint64_t(15);
}
uint32_t ckpt_rec(uint32_t id, int W);                       // bytes per record of a section (0: unknown id)
uint64_t ckpt_count(uint32_t id, const CkptDims& d, bool* fixed);  // the count the dims imply (*fixed false: free, e.g. the host blob)
const char* ckpt_name(uint32_t id);
uint64_t ckpt_sum(const unsigned char* p, uint64_t bytes);   // the checksum rule on the CPU
uint64_t ckpt_head_sum(const unsigned char* file, uint64_t head_bytes);

struct CkptView {
  CkptHead head;
  vg_config cfg;
  std::vector<CkptSec> sec;
  const CkptSec* find(uint32_t id) const {
    for (const CkptSec& s : sec)
      if (s.id == id) return &s;
    return nullptr;
  }
};
// Everything that can be checked without the payload: magic and version, the
// configuration (when cfg != nullptr), the section table's bounds and the
// file length. 0 = ok; else *err names the failed check.
int ckpt_validate(const unsigned char* file, uint64_t len, const vg_config* cfg, CkptView* out, std::string* err);
// ... and the payload: every section's checksum recomputed on the CPU (the
// device does the same in vg_checkpoint_load; this is the tools' and tests' copy)
int ckpt_verify_sums(const unsigned char* file, const CkptView& v, std::string* err);

// bounds-checked reader / writer of the host mirror's blob
struct BlobW {
  std::vector<unsigned char>& b;
  void raw(const void* p, size_t n) { b.insert(b.end(), (const unsigned char*)p, (const unsigned char*)p + n); }
  void i64(int64_t v) { raw(&v, 8); }
  void f64(double v) { raw(&v, 8); }
  void f64s(const double* p, size_t n) { raw(p, n * 8); }
};
struct BlobR {
  const unsigned char* p;
  size_t n, at = 0;
  bool ok = true;
  bool raw(void* out, size_t k) {
    if (!ok || k > n - at) return ok = false;
    memcpy(out, p + at, k);
    at += k;
    return true;
  }
  int64_t i64() {
    int64_t v = 0;
    raw(&v, 8);
    return v;
  }
  double f64() {
    double v = 0;
    raw(&v, 8);
    return v;
  }
  // a count that the remaining bytes can hold `each` bytes of (else the reader fails)
  size_t count(size_t each, size_t limit) {
    const int64_t v = i64();
    if (!ok || v < 0 || (uint64_t)v > limit || (each > 0 && (uint64_t)v > (n - at) / each)) {
      ok = false;
      return 0;
    }
    return (size_t)v;
  }
};

}  // namespace vg
