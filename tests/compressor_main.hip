// Stand-alone device run of compressor_kernel (graphaudio_amd/csrc/ga_dynamics.hip; DynamicsCompressorNode)
// through launch_compressor, the launcher the library uses.  The truth is not here: tests/test_gpu_compressor_kernel.py writes the
// case, runs this program and compares what it wrote with the float64 model of tests/_compressor_model.py.
//
//   compressor_check <case.bin> <out.bin> <n0,n1,...>
//
// case.bin: int32 nodes, int32 blocks; per node: int32 nch[blocks] (0 = a silent block, 1, 2), float params[blocks][6] (the six
// parameter values in GA_COMPRESSOR_* order, clamped), float x[2][blocks * 128].  Sample rate 48000.
// The blocks [0, n0 + n1 + ...) are rendered as one launch per n_i over all nodes, yL carried in device memory from launch to
// launch, as a render cut into chunks of those lengths: every launch gets tables of its own (the chunk's blocks re-indexed from 0,
// one parameter entry per block), one job per node whose segments are the runs of equal channel count -- the planner's layout.
// out.bin: per node float y[2][blocks * 128] (0xCD bytes where nothing was written: silent blocks, channel 1 of mono blocks, blocks
// behind the rendered ones), then double yL[nodes].  Before every launch the program checks, on the host, that every frame a job reads
// or writes lies inside the node's rows.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ga_kernels.hpp"

using namespace ga;

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::printf("usage: compressor_check case.bin out.bin n0,n1,...\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[2];
  if (std::fread(hdr, 4, 2, f) != 2 || hdr[0] < 1 || hdr[0] > 64 || hdr[1] < 1 || hdr[1] > 4096) { std::printf("bad header\n"); return 2; }
  const int nodes = hdr[0], blocks = hdr[1];
  const size_t frames = (size_t)blocks * kBlock;
  std::vector<std::vector<int32_t>> nch(nodes);
  std::vector<std::vector<float>> par(nodes), x(nodes);
  for (int k = 0; k < nodes; k++) {
    if (!read_n(f, nch[k], (size_t)blocks) || !read_n(f, par[k], (size_t)blocks * 6) || !read_n(f, x[k], 2 * frames)) { std::printf("short file\n"); return 2; }
    for (int32_t c : nch[k])
      if (c < 0 || c > 2) { std::printf("bad channel count\n"); return 2; }
  }
  std::fclose(f);
  std::vector<int> split;
  int total = 0;
  for (const char* p = argv[3]; *p;) {
    char* e;
    const long v = std::strtol(p, &e, 10);
    if (e == p || v < 1) { std::printf("bad split\n"); return 2; }
    split.push_back((int)v);
    total += (int)v;
    p = *e == ',' ? e + 1 : e;
  }
  if (total > blocks) { std::printf("split longer than the case\n"); return 2; }

  float *dx = nullptr, *dy = nullptr;
  double* dstate = nullptr;
  CK(hipMalloc(&dx, (size_t)nodes * 2 * frames * sizeof(float)));
  CK(hipMalloc(&dy, (size_t)nodes * 2 * frames * sizeof(float)));
  CK(hipMalloc(&dstate, nodes * sizeof(double)));
  for (int k = 0; k < nodes; k++) CK(hipMemcpy(dx + (size_t)k * 2 * frames, x[k].data(), 2 * frames * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemset(dy, 0xCD, (size_t)nodes * 2 * frames * sizeof(float)));
  CK(hipMemset(dstate, 0, nodes * sizeof(double)));

  int c0 = 0, launches = 0;
  for (int n : split) {   // one chunk: blocks [c0, c0 + n) of the case are blocks [0, n) of the chunk
    std::vector<uint8_t> tab;
    auto put = [&](const void* p, size_t bytes) {
      const size_t off = (tab.size() + 15) & ~(size_t)15;
      tab.resize(off + bytes);
      std::memcpy(&tab[off], p, bytes);
      return off;
    };
    std::vector<CompressorJob> jobs;
    for (int k = 0; k < nodes; k++) {
      std::vector<CompressorParams> pt((size_t)n);
      for (int b = 0; b < n; b++) pt[(size_t)b] = compressor_params(&par[k][(size_t)(c0 + b) * 6], 48000.0);
      std::vector<CompressorSeg> sg;
      for (int b = 0; b < n;) {
        int e = b;
        while (e < n && nch[k][c0 + e] == nch[k][c0 + b]) e++;
        CompressorSeg s{};
        s.b0 = b;
        s.nb = e - b;
        s.nch = nch[k][c0 + b];
        for (int ch = 0; ch < s.nch; ch++) {   // chunk-frame indexed views
          s.in[ch] = dx + ((size_t)k * 2 + ch) * frames + (size_t)c0 * kBlock;
          s.out[ch] = dy + ((size_t)k * 2 + ch) * frames + (size_t)c0 * kBlock;
        }
        // bounds: the segment's frames [b0 * 128, (b0 + nb) * 128) of the chunk are frames of the case
        if (s.b0 < 0 || s.nb < 1 || (size_t)(c0 + s.b0 + s.nb) * kBlock > frames) { std::printf("segment out of bounds\n"); return 1; }
        sg.push_back(s);
        b = e;
      }
      CompressorJob j{};
      j.par_off = put(pt.data(), pt.size() * sizeof(CompressorParams));
      j.seg_off = put(sg.data(), sg.size() * sizeof(CompressorSeg));
      j.state = dstate + k;
      j.nseg = (int)sg.size();
      j.par_stride = 1;
      jobs.push_back(j);
    }
    const size_t joff = put(jobs.data(), jobs.size() * sizeof(CompressorJob));
    uint8_t* dtab = nullptr;
    CK(hipMalloc(&dtab, tab.size()));
    CK(hipMemcpy(dtab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    launch_compressor(0, (const CompressorJob*)(dtab + joff), nodes, dtab);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipFree(dtab));
    c0 += n;
    launches++;
  }

  std::vector<float> y((size_t)nodes * 2 * frames);
  std::vector<double> st((size_t)nodes);
  CK(hipMemcpy(y.data(), dy, y.size() * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(st.data(), dstate, st.size() * sizeof(double), hipMemcpyDeviceToHost));
  FILE* o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(y.data(), sizeof(float), y.size(), o) != y.size() || std::fwrite(st.data(), sizeof(double), st.size(), o) != st.size()) {
    std::printf("cannot write %s\n", argv[2]);
    return 2;
  }
  std::fclose(o);
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dstate);
  std::printf("%d nodes, %d blocks in %d launches\nok\n", nodes, total, launches);
  return 0;
}
