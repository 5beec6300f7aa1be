// rgl_spectral_dir_grad_host_harness.hip — the per-lane function k_rgl_spectral_dir_grad runs (csrc/merl_rgl_spectral_dir_grad.hpp,
// rgl::eval_dir_grad_spectral) and the product's image builder (csrc/merl_rgl.hip) compiled for the HOST, so that
// tests/test_rgl_spectral_dir_grad_cpu.py can hold the gradient of eval on a spectral RGL material to its reference in a container
// without a GPU.  No HIP runtime call is made.  Built by the test with hipcc.  Modelled on tests/rgl_dir_grad_host_harness.hip.
//   usage: rgl_spectral_dir_grad_host_harness <fields.bin> <units.bin> <out.bin> [mask]
//   mask: the per-lane function instantiated for the file's own bracket shape (MASK 1 / 3 / 5 / 15, what the single-material kernels
//         run) instead of MASK 0 (the shape tested at run time, what the id kernel runs)
//   fields.bin: int32 n_phi n_theta nx ny ndf_nx ndf_ny sigma_nx sigma_ny jacobian n_wavelengths, then phi_i theta_i ndf sigma vndf
//               luminance spectra wavelengths (float32); every table [..][ny][nx]
//   units.bin:  uint64 n, int32 W, int32 has_wl, then wi[n][3] wo[n][3] g[n][W] and (has_wl) wavelengths[n][W]
//   out.bin:    grad_wi[n][3] grad_wo[n][3] grad_wavelengths[n][W] (zeros without wavelengths) eval[n][W] (float32)
#include "../mitsuba_customization_amd/csrc/merl_rgl.hip"
#include "../mitsuba_customization_amd/csrc/merl_rgl_spectral_dir_grad.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int h[10];
    if (std::fread(h, 4, 10, f) != 10) return 3;
    mrl::RglFields F;
    F.n_phi = h[0]; F.n_theta = h[1]; F.res[0] = h[2]; F.res[1] = h[3]; F.res_ndf[0] = h[4]; F.res_ndf[1] = h[5]; F.res_sigma[0] = h[6]; F.res_sigma[1] = h[7];
    F.jacobian = h[8]; F.n_wl = h[9]; F.wavelengths = nullptr;
    if (F.n_wl < 1 || mrl::rgl_check_shapes(F)) return 3;
    std::vector<std::vector<float>> keep;
    bool ok = true;
    auto rd = [&](size_t n) { keep.emplace_back(n); ok = ok && std::fread(keep.back().data(), 4, n, f) == n; return keep.back().data(); };
    const size_t per = (size_t)F.res[0] * F.res[1], sl = (size_t)F.n_phi * F.n_theta;
    F.phi_i = rd(F.n_phi); F.theta_i = rd(F.n_theta); F.ndf = rd((size_t)F.res_ndf[0] * F.res_ndf[1]); F.sigma = rd((size_t)F.res_sigma[0] * F.res_sigma[1]);
    F.vndf = rd(sl * per); F.luminance = rd(sl * per); F.rgb = rd(sl * per * (size_t)F.n_wl); F.wavelengths = rd(F.n_wl);
    std::fclose(f);
    if (!ok) return 3;
    if (const char *why = mrl::rgl_check_fields(F)) { std::fprintf(stderr, "%s\n", why); return 4; }
    std::vector<float> blob;
    const mrl::RglLayout L = mrl::rgl_build_image(F, blob);
    const mrl::RglDev r = mrl::rgl_descriptor(F, L, blob.data());
    f = std::fopen(argv[2], "rb");
    if (!f) return 3;
    unsigned long long n = 0;
    int W = 0, has_wl = 0;
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(&W, 4, 1, f) != 1 || std::fread(&has_wl, 4, 1, f) != 1 || W < 1) return 3;
    if (!has_wl && W != F.n_wl) return 3;
    const size_t rows = (size_t)W * n;
    std::vector<float> wi(3 * n), wo(3 * n), g(rows), wl(has_wl ? rows : 0), out(6 * n + 2 * rows, 0.0f);
    if (std::fread(wi.data(), 4, 3 * n, f) != 3 * n || std::fread(wo.data(), 4, 3 * n, f) != 3 * n || std::fread(g.data(), 4, rows, f) != rows) return 3;
    if (has_wl && std::fread(wl.data(), 4, rows, f) != rows) return 3;
    std::fclose(f);
    const mrl::rgl::GridMem grids{ r.phi, r.theta, r.wavelengths };
    float *gwl = &out[6 * n], *ev = &out[6 * n + rows];
    const bool own = argc >= 5 && !std::strcmp(argv[4], "mask");
    const int mask = own ? (1 | (r.n_phi > 1 ? 2 : 0) | (r.n_theta > 1 ? 4 : 0) | (r.n_phi > 1 && r.n_theta > 1 ? 8 : 0)) : 0;
    auto unit = [&](auto m, size_t i, const float *wl_row) {
        return mrl::rgl::eval_dir_grad_spectral<decltype(m)::value>(r, grids, wi[3 * i], wi[3 * i + 1], wi[3 * i + 2], wo[3 * i], wo[3 * i + 1], wo[3 * i + 2],
                                                                    &g[(size_t)W * i], wl_row, W, has_wl ? gwl + (size_t)W * i : nullptr);
    };
    for (size_t i = 0; i < n; ++i) {
        const float *wl_row = has_wl ? &wl[(size_t)W * i] : nullptr;
        mrl::rgl::RglDirGrad d;
        switch (mask) {
        case 1:  d = unit(std::integral_constant<int, 1>{}, i, wl_row); break;
        case 3:  d = unit(std::integral_constant<int, 3>{}, i, wl_row); break;
        case 5:  d = unit(std::integral_constant<int, 5>{}, i, wl_row); break;
        case 15: d = unit(std::integral_constant<int, 15>{}, i, wl_row); break;
        default: d = unit(std::integral_constant<int, 0>{}, i, wl_row); break;
        }
        float pdf;
        for (int k = 0; k < 3; ++k) { out[3 * i + k] = d.wi[k]; out[3 * n + 3 * i + k] = d.wo[k]; }
        mrl::rgl::eval_pdf_spectral<true, false>(r, wi[3 * i], wi[3 * i + 1], wi[3 * i + 2], wo[3 * i], wo[3 * i + 1], wo[3 * i + 2], wl_row, W, ev + (size_t)W * i, pdf);
    }
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 5;
    std::fclose(f);
    std::printf("rgl spectral direction-gradient host harness ok: %llu units x %d wavelengths, MASK %d\n", n, W, mask);
    return 0;
}
