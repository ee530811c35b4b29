// ckpt_check — the checkpoint file's host-side validator as a stand-alone
// program (csrc/ckpt_file.cpp, no GPU): `ckpt_check FILE...` validates each
// file (header, section table, file length, every checksum) and prints the
// verdict; `ckpt_check --selftest` builds a small valid file in memory and
// feeds the validator its malformed variants (a flipped payload byte, a
// truncated file, a bad magic, another configuration, truncated and over-long
// section tables, sections out of bounds). Meant for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -o ckpt_check tools/ckpt_check.cpp csrc/ckpt_file.cpp
#include <cstdio>
#include <cstdlib>
#include "../csrc/ckpt_file.h"

using namespace vg;

static int check(const std::vector<unsigned char>& f, const vg_config* cfg, std::string* why) {
  CkptView v;
  if (ckpt_validate(f.data(), f.size(), cfg, &v, why) != 0) return -1;
  return ckpt_verify_sums(f.data(), v, why);
}

// a valid file of an empty map: every section present, a few with payload
static std::vector<unsigned char> make_file(const vg_config& cfg) {
  CkptHead h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, kCkptMagic, 8);
  h.version = kCkptVersion;
  h.cfg_bytes = sizeof(vg_config);
  h.dims.W = cfg.win_size;
  h.dims.cap_wp = 1000;
  h.dims.max_layer = cfg.max_layer;
  h.dims.n_nodes = 3;
  h.dims.n_roots = 1;
  std::vector<CkptSec> sec;
  std::vector<unsigned char> img;
  for (uint32_t id = kSecHdr; id < kSecEnd; id++) {
    CkptSec s;
    memset(&s, 0, sizeof(s));
    s.id = id;
    s.rec = ckpt_rec(id, h.dims.W);
    bool fixed = false;
    s.count = ckpt_count(id, h.dims, &fixed);
    if (!fixed) s.count = 13;  // the host blob: any length, here no multiple of 8
    s.bytes = s.count * s.rec;
    s.off = img.size();
    for (uint64_t i = 0; i < s.bytes; i++) img.push_back((unsigned char)(i * 37 + id));
    while (img.size() % 16) img.push_back(0);
    s.sum = ckpt_sum(img.data() + s.off, s.bytes);
    sec.push_back(s);
  }
  h.nsec = (uint32_t)sec.size();
  h.head_bytes = (uint32_t)ckpt_head_bytes(h.nsec);
  h.image_bytes = img.size();
  std::vector<unsigned char> f(h.head_bytes, 0);
  memcpy(f.data(), &h, sizeof(h));
  memcpy(f.data() + sizeof(h), &cfg, sizeof(cfg));
  memcpy(f.data() + sizeof(h) + sizeof(cfg), sec.data(), sec.size() * sizeof(CkptSec));
  h.head_sum = ckpt_head_sum(f.data(), h.head_bytes);
  memcpy(f.data(), &h, sizeof(h));
  f.insert(f.end(), img.begin(), img.end());
  return f;
}

static void reseal(std::vector<unsigned char>& f) {  // a tampered header with a matching header checksum
  CkptHead h;
  memcpy(&h, f.data(), sizeof(h));
  const uint64_t hb = ckpt_head_bytes(h.nsec <= (uint32_t)kCkptMaxSec ? h.nsec : 0);
  if (hb > f.size()) return;
  h.head_sum = ckpt_head_sum(f.data(), hb);
  memcpy(f.data(), &h, sizeof(h));
}

static int selftest() {
  vg_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.voxel_size = 1.0;
  cfg.win_size = 10;
  cfg.max_layer = 2;
  const std::vector<unsigned char> good = make_file(cfg);
  std::string why;
  int bad = 0;
  auto expect = [&](const char* name, const std::vector<unsigned char>& f, const vg_config* c, const char* word) {
    std::string w;
    const int r = check(f, c, &w);
    const bool ok = word ? (r != 0 && w.find(word) != std::string::npos) : r == 0;
    printf("%-28s %s%s%s\n", name, ok ? "ok" : "FAILED", w.empty() ? "" : ": ", w.c_str());
    if (!ok) bad++;
  };
  expect("valid", good, &cfg, nullptr);
  CkptHead h;
  memcpy(&h, good.data(), sizeof(h));
  const size_t tab = sizeof(CkptHead) + sizeof(vg_config);
  {
    std::vector<unsigned char> f = good;
    f[h.head_bytes + 40] ^= 0x40;
    expect("flipped payload byte", f, &cfg, "checksum of section");
  }
  for (size_t cut : {size_t(1), size_t(100), good.size() - h.head_bytes, good.size() - 20, good.size()}) {
    std::vector<unsigned char> f(good.begin(), good.end() - (long)cut);
    expect("truncated", f, &cfg, "file length");
  }
  {
    std::vector<unsigned char> f = good;
    f[0] ^= 0xff;
    expect("bad magic", f, &cfg, "magic");
  }
  {
    vg_config other = cfg;
    other.voxel_size = 2.0;
    expect("another voxel_size", good, &other, "config");
  }
  {
    std::vector<unsigned char> f = good;
    f.push_back(0);
    expect("over-long file", f, &cfg, "file length");
  }
  for (uint32_t nsec : {0u, 1u, h.nsec - 1, h.nsec + 1, 65u, 0xffffffffu}) {  // truncated and over-long section tables
    std::vector<unsigned char> f = good;
    CkptHead t = h;
    t.nsec = nsec;
    memcpy(f.data(), &t, sizeof(t));
    expect("section table length", f, &cfg, "section table");
    t.head_bytes = (uint32_t)ckpt_head_bytes(nsec <= 64 ? nsec : 64);
    memcpy(f.data(), &t, sizeof(t));
    reseal(f);
    expect("section table length (sealed)", f, &cfg, "");
  }
  for (int field = 0; field < 3; field++) {  // one entry pointing out of the image, resealed
    std::vector<unsigned char> f = good;
    CkptSec s;
    memcpy(&s, f.data() + tab + 5 * sizeof(CkptSec), sizeof(s));
    if (field == 0) s.off = h.image_bytes + 16;
    if (field == 1) s.bytes = s.count = ~0ull / 2;
    if (field == 2) s.off = ~0ull & ~15ull;
    memcpy(f.data() + tab + 5 * sizeof(CkptSec), &s, sizeof(s));
    reseal(f);
    expect("section out of bounds", f, &cfg, "section table");
  }
  {
    std::vector<unsigned char> f = good;
    CkptHead t = h;
    t.dims.wpn[3] = 2000;  // more window points than a slot holds
    memcpy(f.data(), &t, sizeof(t));
    reseal(f);
    expect("dimensions", f, &cfg, "dimensions");
  }
  printf(bad ? "selftest FAILED (%d)\n" : "selftest ok\n", bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: ckpt_check --selftest | FILE...\n");
    return 2;
  }
  if (std::string(argv[1]) == "--selftest") return selftest();
  int rc = 0;
  for (int i = 1; i < argc; i++) {
    FILE* fp = fopen(argv[i], "rb");
    if (!fp) {
      printf("%s: cannot open\n", argv[i]);
      rc = 1;
      continue;
    }
    std::vector<unsigned char> f;
    unsigned char buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) f.insert(f.end(), buf, buf + k);
    fclose(fp);
    std::string why;
    const int r = check(f, nullptr, &why);
    printf("%s: %s\n", argv[i], r == 0 ? "ok" : why.c_str());
    if (r != 0) rc = 1;
  }
  return rc;
}
