// Batch plan of the BEP 52 device recheck: which bytes of which files share one staging slot,
// and where every leaf digest goes so that ONE launch per tree level serves every unit of the
// batch. Plain C++ (no HIP): gpu_sha256_merkle.hip carries the plan out on the device, and
// module.cpp binds it as _native.merkle_plan so it can be checked where there is no device.
//
// A UNIT is one piece of a file longer than piece_len, or one whole file no longer than
// piece_len. Its WIDTH is piece_len / 16384 for a piece and pow2_ceil(ceil(length / 16384))
// for a small file (BEP 52 pads a small file to the next power of two, not to the piece). Its
// NODE is the root over its leaves completed with zero leaves up to the width: the piece-layer
// entry of a piece, the `pieces root` of a small file.
//
// Data side: units in file order; every file's first byte in the slot at a multiple of 256
// (the leaf kernel loads 16 bytes at a time), a file's pieces back to back. A batch closes when
// the next unit's bytes would pass batch_bytes or the sum of widths would pass
// batch_bytes / 16384 (the capacity of the digest buffers); a large file splits between
// batches at a piece boundary only.
//
// Digest side: units sorted by width, descending and stable. Unit u's leaves go to
// o_u = (sum of the widths before it) in the level-0 buffer. All widths are powers of two and
// every earlier width is at least W_u, so o_u is a multiple of W_u, and at level lv the units
// still being reduced (W >= 2^(lv+1)) are a contiguous prefix whose nodes sit at o_u >> lv. A
// level is then the uniform out[i] = sha256(in[2i] || in[2i+1]) over n_pairs outputs, and the
// units that finish there (W == 2^(lv+1)) are the tail of the prefix, one output each: output
// fin_start + k is the node of sorted unit unit_base + k. Width-1 units finish at the leaf
// level: they are the last w1_count entries of the level-0 buffer and of the sorted order.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <vector>

namespace stager {
namespace merkle_plan {

constexpr int64_t kLeaf = 16384;   // BEP 52 block size
constexpr int64_t kAlign = 256;    // slot alignment of a file's first byte

struct Unit {          // file order
  int64_t file;        // index into the caller's file list
  int64_t piece;       // piece index inside the file (0 for a small file)
  int64_t width;       // leaves of its subtree, a power of two
  int64_t slot_off;    // first byte in the slot
  int64_t bytes;       // data bytes (1 .. piece_len)
};
struct Leaf {          // one per present leaf; the layout the leaf kernel reads (16 bytes)
  int64_t src;         // byte offset in the slot, a multiple of 16
  int32_t len;         // 1 .. 16384
  int32_t dst;         // index in the level-0 digest buffer
};
struct Read {
  int64_t file, file_off, len, slot_off;
};
struct Level {
  int64_t n_pairs;     // outputs of this level's launch
  int64_t fin_start;   // first output that is a finished node
  int64_t unit_base;   // sorted index of the first unit finishing here
};
struct Batch {
  int64_t first_unit = 0;     // index of units[0] among all units of the call
  int64_t data_bytes = 0;     // slot bytes in use (end of the last unit)
  int64_t width_sum = 0;      // level-0 digests, missing leaves included
  int64_t w1_count = 0;       // units of width 1
  std::vector<Unit> units;
  std::vector<Leaf> leaves;
  std::vector<Read> reads;
  std::vector<Level> levels;  // levels[lv] reduces level lv to lv + 1
  std::vector<int64_t> order; // sorted position -> index into units (the inverse permutation)
};

inline int64_t pow2_ceil(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

inline int64_t unit_count(int64_t length, int64_t piece_len) {
  return length > piece_len ? (length + piece_len - 1) / piece_len : 1;
}

class Planner {
 public:
  Planner(std::vector<int64_t> lengths, int64_t piece_len, int64_t batch_bytes)
      : lengths_(std::move(lengths)), piece_len_(piece_len), batch_bytes_(batch_bytes) {
    if (piece_len < kLeaf || (piece_len & (piece_len - 1)))
      throw std::invalid_argument("piece_len must be a power of two, at least 16384");
    if (piece_len > batch_bytes)
      throw std::invalid_argument("piece_len exceeds batch_bytes");
    if (lengths_.empty()) throw std::invalid_argument("no files");
    for (int64_t n : lengths_)
      if (n <= 0) throw std::invalid_argument("a file length must be > 0");
  }

  // The next batch into `b` (its vectors are reused); false when every unit has been planned.
  bool next(Batch& b) {
    b.units.clear();
    b.leaves.clear();
    b.reads.clear();
    b.levels.clear();
    b.order.clear();
    b.first_unit = unit_no_;
    b.data_bytes = b.width_sum = b.w1_count = 0;
    if (file_ >= lengths_.size()) return false;
    const int64_t cap = batch_bytes_ / kLeaf;
    int64_t pos = 0;
    bool full = false;
    while (!full && file_ < lengths_.size()) {
      const int64_t len = lengths_[file_];
      const bool small = len <= piece_len_;
      const int64_t np = unit_count(len, piece_len_);
      const int64_t width = small ? pow2_ceil((len + kLeaf - 1) / kLeaf) : piece_len_ / kLeaf;
      Read rd{(int64_t)file_, piece_ * piece_len_, 0, (pos + kAlign - 1) / kAlign * kAlign};
      while (piece_ < np) {
        const int64_t bytes = small ? len : std::min(piece_len_, len - piece_ * piece_len_);
        const int64_t at = rd.slot_off + rd.len;
        if (!b.units.empty() && (at + bytes > batch_bytes_ || b.width_sum + width > cap)) {
          full = true;  // the unit starts the next batch
          break;
        }
        b.units.push_back(Unit{(int64_t)file_, piece_, width, at, bytes});
        b.width_sum += width;
        rd.len += bytes;
        ++piece_;
      }
      if (rd.len) {
        b.reads.push_back(rd);
        pos = rd.slot_off + rd.len;
      }
      if (piece_ == np) ++file_, piece_ = 0;
    }
    b.data_bytes = pos;
    unit_no_ += (int64_t)b.units.size();
    layout(b);
    return true;
  }

 private:
  static void layout(Batch& b) {
    const size_t n = b.units.size();
    b.order.resize(n);
    std::iota(b.order.begin(), b.order.end(), (int64_t)0);
    std::stable_sort(b.order.begin(), b.order.end(), [&](int64_t x, int64_t y) {
      return b.units[(size_t)x].width > b.units[(size_t)y].width;
    });
    std::vector<int64_t> off(n);  // level-0 offset per unit (file order)
    int64_t o = 0;
    for (int64_t u : b.order) {
      off[(size_t)u] = o;
      o += b.units[(size_t)u].width;
    }
    for (size_t u = 0; u < n; ++u) {
      const Unit& un = b.units[u];
      if (un.width == 1) ++b.w1_count;
      for (int64_t k = 0; k * kLeaf < un.bytes; ++k)
        b.leaves.push_back(Leaf{un.slot_off + k * kLeaf,
                                (int32_t)std::min(kLeaf, un.bytes - k * kLeaf),
                                (int32_t)(off[u] + k)});
    }
    // One pass over the sorted units per level: the prefix with W > T and the one with W >= T.
    const int64_t top = b.units[(size_t)b.order[0]].width;
    size_t j_above = 0, j_active = 0;        // units with W > T / W >= T, T descending below
    int64_t w_above = 0, w_active = 0;
    std::vector<Level> rev;
    int lv = 0;
    while (((int64_t)2 << lv) <= top) ++lv;  // levels 0 .. lv - 1
    for (int l = lv - 1; l >= 0; --l) {
      const int64_t t = (int64_t)2 << l;
      while (j_above < n && b.units[(size_t)b.order[j_above]].width > t)
        w_above += b.units[(size_t)b.order[j_above++]].width;
      if (j_active < j_above) j_active = j_above, w_active = w_above;
      while (j_active < n && b.units[(size_t)b.order[j_active]].width >= t)
        w_active += b.units[(size_t)b.order[j_active++]].width;
      rev.push_back(Level{w_active >> (l + 1), w_above >> (l + 1), (int64_t)j_above});
    }
    b.levels.assign(rev.rbegin(), rev.rend());
  }

  std::vector<int64_t> lengths_;
  int64_t piece_len_, batch_bytes_;
  size_t file_ = 0;
  int64_t piece_ = 0, unit_no_ = 0;
};

}  // namespace merkle_plan
}  // namespace stager
