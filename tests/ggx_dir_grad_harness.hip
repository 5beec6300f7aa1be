// ggx_dir_grad_harness.hip — the product's per-lane direction gradient (csrc/merl_ggx_fast.hpp, fast::ggx_eval_dir_grad: the SAME
// __host__ __device__ function k_ggx_grad_dir runs) compiled for the HOST, so that tests/test_ggx_dir_grad_cpu.py can compare it with
// tests/ggx_dir_grad_reference.py without a GPU.  No HIP runtime call is made.  Built by the test with hipcc.
//   usage: ggx_dir_grad_harness <in.bin> <out.bin>
//   in.bin:  uint64 n, double alpha eta[3] k[3] (the material's stored Float parameters), then wi[n][3] wo[n][3] g[n][3] (float32)
//   out.bin: grad_wi[n][3] grad_wo[n][3] (float32)
#include "../mitsuba_customization_amd/csrc/merl_ggx_fast.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    unsigned long long n = 0;
    double p[7];
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(p, 8, 7, f) != 7) return 3;
    std::vector<float> wi(3 * n), wo(3 * n), g(3 * n), gwi(3 * n), gwo(3 * n);
    if (std::fread(wi.data(), 4, 3 * n, f) != 3 * n || std::fread(wo.data(), 4, 3 * n, f) != 3 * n || std::fread(g.data(), 4, 3 * n, f) != 3 * n) return 3;
    std::fclose(f);
    const mrl::fast::GgxConsts consts = mrl::fast::ggx_consts_exact(p[0], p + 1, p + 4);
    for (size_t i = 0; i < n; ++i) {
        const mrl::fast::GgxDirGrad r = mrl::fast::ggx_eval_dir_grad(consts, wi[3 * i], wi[3 * i + 1], wi[3 * i + 2],
                                                                     wo[3 * i], wo[3 * i + 1], wo[3 * i + 2], &g[3 * i]);
        for (int c = 0; c < 3; ++c) { gwi[3 * i + c] = r.wi[c]; gwo[3 * i + c] = r.wo[c]; }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = std::fwrite(gwi.data(), 4, 3 * n, f) == 3 * n && std::fwrite(gwo.data(), 4, 3 * n, f) == 3 * n;
    return std::fclose(f) == 0 && ok ? 0 : 3;
}
