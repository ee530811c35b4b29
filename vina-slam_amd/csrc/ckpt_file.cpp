// ckpt_file.cpp — the checkpoint file's host-side validator (ckpt_file.h).
// Host-only: no HIP call, no context; every read of the file is bounds-checked
// against its length first.
#include "ckpt_file.h"

namespace vg {

uint32_t ckpt_rec(uint32_t id, int W) {
  switch (id) {
    case kSecHdr: return 96;
    case kSecPlane: return 224;
    case kSecPcrAdd: case kSecPcrFix: return 80;
    case kSecCovAdd: return 45 * 8;
    case kSecEig: return 12 * 8;
    case kSecJour: return 8;
    case kSecDbox: return 6 * 8;
    case kSecPcrs: return (uint32_t)W * 80;
    case kSecLseg: return (uint32_t)W * 8;
    case kSecInSlide: return 1;
    case kSecSlide: return 4;
    case kSecFixPnt: return 24;
    case kSecFixVar: return 72;
    case kSecWpPnt: return 24;
    case kSecWpVar: return 72;
    case kSecWpLeaf: case kSecWpInt: case kSecWpOrd: return 4;
    case kSecSlots: return 4;
    case kSecRootId: return 4;
    case kSecRootKey: return 8;
    case kSecDState: return 8;
    case kSecHost: return 1;
    default: return 0;
  }
}

uint64_t ckpt_count(uint32_t id, const CkptDims& d, bool* fixed) {
  *fixed = true;
  uint64_t wp = 0, ord = 0;
  for (int s = 0; s < 32; s++) {
    wp += (uint64_t)d.wpn[s];
    ord += (uint64_t)d.ord0[s] + (uint64_t)(d.arena[s] > d.cap_wp ? d.arena[s] - d.cap_wp : 0);
  }
  switch (id) {
    case kSecHdr: case kSecPlane: case kSecPcrAdd: case kSecPcrFix: case kSecCovAdd: case kSecEig: case kSecJour:
    case kSecDbox: case kSecPcrs: case kSecLseg: case kSecInSlide:
      return (uint64_t)d.n_nodes;
    case kSecSlide: return (uint64_t)d.n_slide;
    case kSecFixPnt: case kSecFixVar: return (uint64_t)d.n_fix;
    case kSecWpPnt: case kSecWpVar: case kSecWpLeaf: case kSecWpInt: return wp;
    case kSecWpOrd: return ord;
    case kSecSlots: return kCkptSlotInts;
    case kSecRootId: case kSecRootKey: return (uint64_t)d.n_roots;
    case kSecDState: return kCkptDStateDoubles;
    default: *fixed = false; return 0;
  }
}

const char* ckpt_name(uint32_t id) {
  static const char* names[] = {"?", "hdr", "plane", "pcr_add", "pcr_fix", "cov_add", "eig", "jour", "dbox", "pcrs",
                                "lseg", "in_slide", "slide", "fix_pnt", "fix_var", "wp_pnt", "wp_var", "wp_leaf",
                                "wp_int", "wp_ord", "slots", "root_id", "root_key", "dstate", "host"};
  return id < kSecEnd ? names[id] : "?";
}

uint64_t ckpt_sum(const unsigned char* p, uint64_t bytes) {
  uint64_t acc = 0;
  const uint64_t full = bytes / 8;
  for (uint64_t i = 0; i < full; i++) {
    uint64_t w;
    memcpy(&w, p + i * 8, 8);
    acc += w * (kCkptMul * (2 * i + 1));
  }
  if (bytes % 8) {
    uint64_t w = 0;
    memcpy(&w, p + full * 8, bytes % 8);
    acc += w * (kCkptMul * (2 * full + 1));
  }
  return acc;
}

uint64_t ckpt_head_sum(const unsigned char* file, uint64_t head_bytes) {
  std::vector<unsigned char> h(file, file + head_bytes);
  memset(h.data() + offsetof(CkptHead, head_sum), 0, 8);
  return ckpt_sum(h.data(), head_bytes);
}

int ckpt_validate(const unsigned char* file, uint64_t len, const vg_config* cfg, CkptView* out, std::string* err) {
  auto fail = [&](const std::string& what) {
    *err = "checkpoint rejected: " + what;
    return -1;
  };
  if (len < sizeof(CkptHead)) return fail("file length (shorter than the header)");
  CkptHead& h = out->head;
  memcpy(&h, file, sizeof(h));
  if (memcmp(h.magic, kCkptMagic, 8) != 0) return fail("magic");
  if (h.version != kCkptVersion) return fail("version " + std::to_string(h.version));
  if (h.cfg_bytes != sizeof(vg_config)) return fail("config size");
  if (len < sizeof(CkptHead) + sizeof(vg_config)) return fail("file length (shorter than the configuration)");
  memcpy(&out->cfg, file + sizeof(CkptHead), sizeof(vg_config));
  if (cfg && memcmp(cfg, &out->cfg, sizeof(vg_config)) != 0) return fail("config differs from the context's");
  if (h.nsec == 0 || h.nsec > (uint32_t)kCkptMaxSec) return fail("section table (count " + std::to_string(h.nsec) + ")");
  if (h.head_bytes != ckpt_head_bytes(h.nsec)) return fail("section table (header size)");
  if (len < h.head_bytes) return fail("file length (section table truncated)");
  if (h.image_bytes != len - h.head_bytes)
    return fail("file length (" + std::to_string(len) + " bytes, header says " +
                std::to_string(h.head_bytes + h.image_bytes) + ")");
  if (ckpt_head_sum(file, h.head_bytes) != h.head_sum) return fail("header checksum");
  const CkptDims& d = h.dims;
  if (d.W < 1 || d.W > 32 || d.W != out->cfg.win_size || d.max_layer != out->cfg.max_layer || d.cap_wp < 1 ||
      d.n_nodes < 0 || d.n_fix < 0 || d.n_slide < 0 || d.n_roots < 0 || d.n_roots > d.n_nodes || d.n_slide > d.n_nodes)
    return fail("dimensions");
  for (int s = 0; s < 32; s++) {
    const int64_t top = (int64_t)d.cap_wp * (d.max_layer + 1);
    if (d.wpn[s] < 0 || d.wpn[s] > d.cap_wp || (d.arena[s] != 0 && (d.arena[s] < d.cap_wp || d.arena[s] > top)) ||
        d.ord0[s] < 0 || d.ord0[s] > d.wpn[s] || (s >= d.W && (d.wpn[s] || d.arena[s])))
      return fail("dimensions (window slot " + std::to_string(s) + ")");
  }
  out->sec.resize(h.nsec);
  memcpy(out->sec.data(), file + sizeof(CkptHead) + sizeof(vg_config), (size_t)h.nsec * sizeof(CkptSec));
  uint64_t end = 0, seen = 0;
  for (const CkptSec& s : out->sec) {
    const std::string nm = std::string("section table (") + ckpt_name(s.id) + ")";
    const uint32_t rec = ckpt_rec(s.id, d.W);
    if (rec == 0 || s.id >= 64 || s.rec != rec) return fail(nm + ": unknown id or record size");
    if (seen & (1ull << s.id)) return fail(nm + ": listed twice");
    seen |= 1ull << s.id;
    if (s.count > (1ull << 40) || s.bytes != s.count * rec) return fail(nm + ": byte count");
    if ((s.off & 15) || s.off < end || s.off > h.image_bytes || s.bytes > h.image_bytes - s.off)
      return fail(nm + ": out of the image's bounds");
    bool fixed = false;
    const uint64_t want = ckpt_count(s.id, d, &fixed);
    if (fixed && want != s.count) return fail(nm + ": count does not match the dimensions");
    end = s.off + s.bytes;
  }
  for (uint32_t id = kSecHdr; id < kSecEnd; id++)
    if (!(seen & (1ull << id))) return fail(std::string("section table (") + ckpt_name(id) + " missing)");
  return 0;
}

int ckpt_verify_sums(const unsigned char* file, const CkptView& v, std::string* err) {
  const unsigned char* img = file + v.head.head_bytes;
  for (const CkptSec& s : v.sec)
    if (ckpt_sum(img + s.off, s.bytes) != s.sum) {
      *err = std::string("checkpoint rejected: checksum of section ") + ckpt_name(s.id);
      return -1;
    }
  return 0;
}

}  // namespace vg
