// Host-only run of the line band descriptor's arithmetic (cube_slam_wu_amd/csrc/cs_lbd.h: the functions the device kernel compiles -- row walk,
// band sums, mean / std, normalisations, binary conversion -- in a plain loop, one line after the other).  No GPU, no HIP runtime call.
// tests/test_lbd_host_cpu.py holds its output to the numpy restatement (tests/lbd_ref.py) bit for bit.
//   lbd_host_check <in> <out>
//   in:  int32 W, H, n | int16 dx[H][W] | int16 dy[H][W] | n records of { float sx, sy, ex, ey, direction; int32 num_pixels }
//   out: float desc72[n][72] | uint8 desc32[n][32]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_lbd.h"

struct Record { float sx, sy, ex, ey, direction; int32_t num_pixels; };

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t hdr[3];
  if (!f || fread(hdr, 4, 3, f) != 3) return 2;
  const int W = hdr[0], H = hdr[1], n = hdr[2];
  if (W < 1 || H < 1 || W > 32767 || H > 32767 || n < 0) return 2;
  const size_t N = (size_t)W * H;
  std::vector<short> dx(N), dy(N);
  std::vector<Record> rec((size_t)n);
  if (fread(dx.data(), 2, N, f) != N || fread(dy.data(), 2, N, f) != N || fread(rec.data(), sizeof(Record), (size_t)n, f) != (size_t)n) return 2;
  fclose(f);
  cs::LbdWeights w;
  cs::lbd_weights(w);
  const cs::LbdMapPlanes m{dx.data(), dy.data()};
  std::vector<float> d72((size_t)n * cs::LBD_FLOATS);
  std::vector<unsigned char> d32((size_t)n * cs::LBD_BYTES);
  for (int i = 0; i < n; i++) {
    const Record& r = rec[i];
    if (r.num_pixels < 0 || r.num_pixels > 32767) return 3;
    const cs::LbdLine L = cs::lbd_line(r.sx, r.sy, r.ex, r.ey, r.direction, r.num_pixels, 0);
    cs::lbd_describe_one(m, W, H, L, w, d72.data() + (size_t)i * cs::LBD_FLOATS, d32.data() + (size_t)i * cs::LBD_BYTES);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(d72.data(), sizeof(float), d72.size(), o) != d72.size() || fwrite(d32.data(), 1, d32.size(), o) != d32.size()) return 2;
  fclose(o);
  printf("%d lines described\n", n);
  return 0;
}
