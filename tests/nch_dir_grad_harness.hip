// nch_dir_grad_harness.hip — the product's per-lane direction gradient on an n-channel table material (csrc/merl_nch_dir_grad.hpp,
// fast::nch_eval_dir_grad: the SAME __host__ __device__ function k_table_grad_dir_nch runs) compiled for the HOST, so that
// tests/test_nch_dir_grad_cpu.py can compare it with tests/nch_dir_grad_reference.py without a GPU.  No HIP runtime call is made and
// the device's table builder is not used: the brick image (merl_nch.hip: a cell's 8 corners x CPAD channels, corner-major, 32 B / 64 B
// / ceil(n_ch / 4) lines of 128 B per cell) is built here from the planar array.
//   usage: nch_dir_grad_harness <in.bin> <out.bin>
//   in.bin:  uint64 n; int32 dims[3], param, lookup, node, cosine (MRL_OPT_COSINE_FACTOR), keep (MRL_OPT_NEGATIVE = 1), n_ch;
//            double scale[n_ch]; double planar[n_ch][dims0][dims1][dims2]; then wi[n][3] wo[n][3] g[n][n_ch] (float32)
//   out.bin: grad_wi[n][3] grad_wo[n][3] (float32)
#include "../mitsuba_customization_amd/csrc/merl_nch_dir_grad.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    unsigned long long n = 0;
    int head[9];
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(head, 4, 9, f) != 9) return 3;
    const int n0 = head[0], n1 = head[1], n2 = head[2], param = head[3], n_ch = head[8];
    if (n0 < 1 || n1 < 1 || n2 < 1 || param < 0 || param > 2 || n_ch < 1 || n_ch > 32 || n_ch == 3) return 4;
    const size_t plane = (size_t)n0 * n1 * n2;
    std::vector<double> scale(n_ch), planar((size_t)n_ch * plane);
    std::vector<float> wi(3 * n), wo(3 * n), g((size_t)n_ch * n), out(6 * n);
    if (std::fread(scale.data(), 8, n_ch, f) != (size_t)n_ch || std::fread(planar.data(), 8, planar.size(), f) != planar.size()) return 3;
    if (std::fread(wi.data(), 4, 3 * n, f) != 3 * n || std::fread(wo.data(), 4, 3 * n, f) != 3 * n || std::fread(g.data(), 4, g.size(), f) != g.size()) return 3;
    std::fclose(f);

    const bool keep = head[7] != 0, periodic = mrl::param_phi_periodic(param);
    // the stored texel of logical index (h, d, p), channel ch: Float(value x scale), negatives clamped to 0 unless kept
    auto texel = [&](int h, int d, int p, int ch) -> float {
        const double v = planar[(size_t)ch * plane + ((size_t)h * n1 + d) * n2 + p] * scale[ch];
        return (v > 0.0 || keep) ? (float)v : 0.0f;
    };
    // corner index -> logical index: the clamped axes repeat their last texel, the periodic azimuth wraps
    auto fold = [](int i, int n_axis, bool wrap) { return i < n_axis ? i : (wrap ? 0 : n_axis - 1); };
    const int cpad = n_ch == 1 ? 1 : n_ch == 2 ? 2 : 4, groups = cpad == 4 ? (n_ch + 3) / 4 : 1, pieces = 2 * cpad;
    std::vector<float4> bricks(plane * groups * pieces);
    for (int h = 0; h < n0; ++h)
        for (int d = 0; d < n1; ++d)
            for (int p = 0; p < n2; ++p)
                for (int grp = 0; grp < groups; ++grp) {
                    float v[32] = { 0.0f };
                    for (int k = 0; k < 8; ++k)
                        for (int ch = 0; ch < cpad; ++ch) {
                            const int c = cpad * grp + ch;
                            // padding channels hold a value no sum may see
                            v[k * cpad + ch] = c < n_ch ? texel(fold(h + (k >> 2), n0, false), fold(d + ((k >> 1) & 1), n1, false), fold(p + (k & 1), n2, periodic), c)
                                                        : 1.0e30f * (float)(k + 1);
                        }
                    float4 *dst = &bricks[((((size_t)h * n1 + d) * n2 + p) * groups + grp) * pieces];
                    for (int q = 0; q < pieces; ++q) dst[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
                }

    mrl::MaterialDev m = {};
    m.kind = mrl::KIND_TABLE_NCH;
    m.n_th = n0; m.n_td = n1; m.n_pd = n2;
    m.n_ch = n_ch;
    m.param = param;
    m.layout = mrl::LAYOUT_BRICK;
    m.texels = bricks.data();
    mrl::Options o = {};
    o.lookup = head[4]; o.node = head[5]; o.cosine = head[6]; o.negative = keep ? 1 : 0;
    float *gwi = out.data(), *gwo = gwi + 3 * n;
    for (size_t i = 0; i < n; ++i) {
        const float *gi = &g[i * (size_t)n_ch];
        const float a0 = wi[3 * i], a1 = wi[3 * i + 1], a2 = wi[3 * i + 2], b0 = wo[3 * i], b1 = wo[3 * i + 1], b2 = wo[3 * i + 2];
        const mrl::fast::TableDirGrad r = cpad == 1 ? mrl::fast::nch_eval_dir_grad<1>(m, o, a0, a1, a2, b0, b1, b2, gi, n_ch)
                                        : cpad == 2 ? mrl::fast::nch_eval_dir_grad<2>(m, o, a0, a1, a2, b0, b1, b2, gi, n_ch)
                                                    : mrl::fast::nch_eval_dir_grad<4>(m, o, a0, a1, a2, b0, b1, b2, gi, n_ch);
        for (int c = 0; c < 3; ++c) { gwi[3 * i + c] = r.wi[c]; gwo[3 * i + c] = r.wo[c]; }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = std::fwrite(out.data(), 4, 6 * n, f) == 6 * n;
    return std::fclose(f) == 0 && ok ? 0 : 3;
}
