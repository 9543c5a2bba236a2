// Host check of csrc/seg_walk.h (tests/test_seg_walk.py builds it with -fsanitize=address,undefined and runs it): the walk
// over random offsets, good and bad, chunk by chunk.  Prints one line per (R, family); exit status 1 on the first violation.
#include "seg_walk.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mtmc;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {                                   // splitmix64: the same draws with every library
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }      // [0, n)

struct Draw { int R, family; int64_t N, D; std::vector<int64_t> offsets; };

[[noreturn]] static void fail(const Draw& d, int64_t r0, const char* what) {
  std::printf("FAIL R=%d family=%d N=%lld D=%lld chunk at %lld: %s\n  offsets:", d.R, d.family, (long long)d.N, (long long)d.D,
              (long long)r0, what);
  for (int64_t v : d.offsets) std::printf(" %lld", (long long)v);
  std::printf("\n");
  std::exit(1);
}

// offsets as the walk sees them: any index outside [0, N] fails, every read is counted
struct Checked {
  const Draw* d;
  int64_t r0;
  long* reads;
  int64_t operator[](int64_t i) const {
    if (i < 0 || i > d->N) fail(*d, r0, "offsets read outside [0, N]");
    ++*reads;
    return d->offsets[(size_t)i];
  }
};

static Draw draw(int R, int family) {
  Draw d;
  d.R = R;
  d.family = family;
  d.N = 1 + below(9);
  d.D = below(5 * R + 3);
  d.offsets.resize((size_t)d.N + 1);
  if (family <= 2) {                                      // sorted inside [0, D]; family 1 with its ends pinned
    for (auto& v : d.offsets) v = below(d.D + 1);
    std::sort(d.offsets.begin(), d.offsets.end());
    if (family == 1) { d.offsets.front() = 0; d.offsets.back() = d.D; }
  } else {
    for (auto& v : d.offsets) {
      v = below(d.D + 5) - 2;                             // [-2, D + 2], any order
      if (family == 4 && below(3) == 0) v = (int64_t)rnd();
    }
  }
  return d;
}

static void check_chunk(const Draw& d, int64_t r0, int64_t r1) {
  long find_reads = 0, reads = 0;
  seg_find(Checked{&d, r0, &find_reads}, d.N, d.D, r0);
  int64_t at = r0;
  std::vector<int64_t> owner((size_t)(r1 - r0), -1);
  const bool sorted = d.family <= 2;
  auto piece = [&](int64_t s, int64_t a, int64_t b, int64_t lo, int64_t hi) {
    if (s < 0 || s >= d.N) fail(d, r0, "piece of a range outside [0, N)");
    if (a != seg_clamp(d.offsets[(size_t)s], d.D) || b != seg_clamp(d.offsets[(size_t)s + 1], d.D)) fail(d, r0, "piece with other ends than its range's");
    if (lo != at || hi <= lo || hi > r1) fail(d, r0, "pieces and gaps do not tile the chunk");
    if (!(a <= lo && hi <= b)) fail(d, r0, "piece outside its range");
    if (sorted && seg_inside(a, b, r0, r1) != (seg_first_chunk(a, d.R) == seg_last_chunk(b, d.R))) fail(d, r0, "chunk side and finish side disagree on a crossing");
    for (int64_t j = lo; j < hi; ++j) owner[(size_t)(j - r0)] = s;
    at = hi;
  };
  auto gap = [&](int64_t lo, int64_t hi) {
    if (lo != at || hi <= lo || hi > r1) fail(d, r0, "pieces and gaps do not tile the chunk");
    at = hi;
  };
  seg_walk(Checked{&d, r0, &reads}, d.N, d.D, r0, r1, piece, gap);
  if (at != r1) fail(d, r0, "the walk ends before the chunk does");
  if ((reads - find_reads) / 2 > d.N + 1) fail(d, r0, "more ranges examined than N + 1");
  if (sorted) {                                           // the owner of j is THE s with offsets[s] <= j < offsets[s + 1]
    for (int64_t j = r0; j < r1; ++j) {
      int64_t want = -1;
      for (int64_t s = 0; s < d.N; ++s) {
        if (d.offsets[(size_t)s] <= j && j < d.offsets[(size_t)s + 1]) want = s;
      }
      if (owner[(size_t)(j - r0)] != want) fail(d, r0, "a position with another owner than the range that holds it");
    }
  }
}

int main(int argc, char** argv) {
  const long draws = argc > 1 ? std::atol(argv[1]) : 100000;
  const int Rs[3] = {4, 32, 64};
  for (int R : Rs) {
    long chunks[5] = {0, 0, 0, 0, 0}, wide[5] = {0, 0, 0, 0, 0};
    for (long i = 0; i < draws; ++i) {
      const Draw d = draw(R, 1 + (int)(i % 4));
      if (seg_chunks(d.D, R) * R < d.D || (seg_chunks(d.D, R) - 1) * R >= d.D + (d.D == 0)) fail(d, 0, "seg_chunks");
      for (int64_t c = 0; c < seg_chunks(d.D, R); ++c) {
        const int64_t r0 = c * R, r1 = seg_chunk_end(r0, R, d.D);
        if (r1 <= r0 || r1 > d.D || r1 - r0 > R) fail(d, r0, "seg_chunk_end");
        check_chunk(d, r0, r1);
        ++chunks[d.family];
        if (d.D >= 2 * R) ++wide[d.family];
      }
    }
    for (int f = 1; f <= 4; ++f) {
      std::printf("R=%d family %d: %ld chunks walked, %ld of them with D >= 2 R\n", R, f, chunks[f], wide[f]);
      if (wide[f] == 0) { std::printf("FAIL: family %d never had D >= 2 R\n", f); return 1; }
    }
  }
  std::printf("ok\n");
  return 0;
}
