// san_keccak.cpp -- a stand-alone host program over csrc/keccak.hpp, the permutation and the sponge
// index algebra of the rg_xof_* kernels, meant to be built with -fsanitize=address,undefined and run on
// the CPU (tests/test_keccak_host.py does both, and writes the case file with hashlib.shake_128).
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I ringo-snark_amd/csrc tools/san_keccak.cpp -o san_keccak && ./san_keccak cases.txt
// A case is one line of three fields:
//   <message chunks, hex, comma-separated, "-" for an empty chunk>  <read sizes, comma-separated>  <output, hex>
// Each chunk is one absorb, each size one squeeze; the reads' bytes, concatenated, must equal the output.
// Every buffer is allocated at its exact size, so a read or write past an end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "keccak.hpp"

namespace kk = rg::keccak;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> v;
  if (h == "-") return v;
  for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
  return v;
}

static std::vector<std::string> split(const std::string& s, char c) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, c)) out.push_back(item);
  return out;
}

// the table identities the cooperative kernel relies on
static int check_tables() {
  int bad = 0;
  bool seen[kk::kWords] = {};
  for (int i = 0; i < kk::kWords; ++i) {
    const int d = kk::pi_dest(i);
    if (d < 0 || d >= kk::kWords || seen[d] || kk::pi_source(d) != i) ++bad;
    if (d >= 0 && d < kk::kWords) seen[d] = true;
  }
  for (int p = 0; p < kk::kRate; ++p) {
    uint64_t w[kk::kRateWords];
    for (int i = 0; i < kk::kRateWords; ++i) w[i] = kk::pad_word(p, i);
    const uint8_t* b = reinterpret_cast<const uint8_t*>(w);  // little-endian host
    for (int q = 0; q < kk::kRate; ++q) {
      const uint8_t want = (uint8_t)((q == p ? kk::kDomain : 0) ^ (q == kk::kRate - 1 ? kk::kFinalBit : 0));
      if (b[q] != want) ++bad;
    }
  }
  if ((kk::pad_word(167, 20) >> 56) != 0x9F) ++bad;  // the domain byte and the final bit coincide
  // a run's blocks tile it
  for (int pos = 0; pos < kk::kRate; pos += 13) {
    for (size_t len : {(size_t)0, (size_t)1, (size_t)167, (size_t)168, (size_t)169, (size_t)1000}) {
      const kk::Run r = kk::split_run(pos, len);
      size_t next = 0;
      for (size_t blk = 0; blk < r.blocks; ++blk) {
        size_t lo, hi;
        kk::block_range(pos, len, blk, lo, hi);
        if (lo != next || hi < lo || hi - lo > (size_t)kk::kRate) ++bad;
        if (kk::word_start(pos, blk, 0) + pos != (long long)(blk * kk::kRate)) ++bad;
        next = hi;
      }
      if (next != len || (size_t)r.end_pos != (pos + len) % kk::kRate) ++bad;
    }
  }
  if (bad) std::printf("tables: %d identities fail\n", bad);
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: san_keccak <case file>\n");
    return 2;
  }
  int bad = check_tables();
  std::ifstream in(argv[1]);
  std::string line;
  int n = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    const std::vector<std::string> f = split(line, ' ');
    if (f.size() != 3) {
      std::printf("case %d: malformed\n", n);
      return 2;
    }
    kk::Sponge s;
    kk::sponge_reset(s);
    for (const std::string& c : split(f[0], ',')) {
      const std::vector<uint8_t> m = unhex(c);
      if (!kk::sponge_absorb(s, m.data(), m.size())) ++bad;
    }
    std::vector<uint8_t> got;
    for (const std::string& r : split(f[1], ',')) {
      std::vector<uint8_t> o(std::stoul(r));
      kk::sponge_squeeze(s, o.data(), o.size());
      got.insert(got.end(), o.begin(), o.end());
    }
    const uint8_t one = 0;
    if (kk::sponge_absorb(s, &one, 1)) ++bad;  // absorbing after a squeeze is refused
    if (got != unhex(f[2])) {
      std::printf("case %d: output differs (chunks %s reads %s)\n", n, f[0].substr(0, 40).c_str(), f[1].substr(0, 40).c_str());
      ++bad;
    }
    ++n;
  }
  if (n == 0) {
    std::printf("no cases\n");
    return 2;
  }
  if (bad) return 1;
  std::printf("keccak ok: %d cases\n", n);
  return 0;
}
