// K2 -- the row launcher of the two-kernel envelope route: one workgroup per (utterance, channel) row, k_envelope of
// f2_envelope_row.h (the algorithm is described there), one instantiation per length class and precision plus the
// three-pass plan of the 1 s row. f2_launch_envelope sorts the utterances of a call by padded length and hands the
// longer ones to f2_envelope_pair.hip, f2_envelope_split.hip and f2_envelope_large.hip, the flagged ones of the
// spectral kernel's classes to f2_envelope_flagged.hip.
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "f2_fft_lds.h"

using namespace f2fft;

namespace {

#include "f2_envelope_row.h"

template <typename F>
using EnvKernel = void (*)(EnvParams, const cpx<F>*);

template <typename F, int... L>
constexpr EnvKernel<F> kernel_table_impl(int log2h, std::integer_sequence<int, L...>) {
    EnvKernel<F> tab[] = {k_envelope<F, L>...};
    return tab[log2h];
}

template <typename F, int MAXL>
EnvKernel<F> kernel_for(int log2h) {
    return kernel_table_impl<F>(log2h, std::make_integer_sequence<int, MAXL + 1>{});
}

constexpr int MAX_LOG2H_F32 = 14;  // rows up to 32768 samples
constexpr int MAX_LOG2H_F64 = 13;  // rows up to 16384 samples

}  // namespace

int f2_launch_envelope(f2_ctx* ctx, const double* d_gfb, const int64_t* d_offsets, const int64_t* h_offsets,
                       int B, int C, int lpf, double cutoff_hz, int precision, double* d_env, const f2_handoff* handoff,
                       const int* d_uflag, const int* h_flag0) {
    const bool f32_in = handoff && handoff->f32;
    F2_CHECK(ctx, !f32_in || precision == F2_FFT_F32, F2_ERR_INVALID, "float32 hand-off needs the float FFT");
    EnvParams P;
    P.f32_in = f32_in ? 1 : 0;
    P.uflag = d_uflag;
    P.stamps = nullptr;
    P.gfb = d_gfb;
    P.env = d_env;
    P.offsets = d_offsets;
    P.C = C;
    P.lpf = lpf ? 1 : 0;
    // butter(1, cutoff/8000): bilinear transform of 1/(s+1), pre-warped (EnvelopeExtraction.py:47)
    const double k = lpf ? tan(3.14159265358979323846 * cutoff_hz / 16000.0) : 0.0;
    P.b0 = k / (1.0 + k);
    P.a1 = (k - 1.0) / (k + 1.0);

    // group the utterances by padded length (one kernel instantiation per FFT size)
    std::vector<std::vector<int>> groups(32), split_groups(32);
    std::vector<int> pair_group[2];   // [1]: 32769..65536 samples, two sub-rows per workgroup (f2_envelope_pair.hip)
    const bool pair_ok = ctx->opt_env_pair && ((f32_in && handoff->d_x32) || (!f32_in && d_gfb != d_env));
    int n_large = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = h_offsets[b + 1] - h_offsets[b];
        if (n <= 0) continue;
        const int log2m = n <= 2 ? 1 : f2_log2_ceil(n);
        const int log2h = log2m - 1;
        const int maxl = precision == F2_FFT_F32 ? MAX_LOG2H_F32 : MAX_LOG2H_F64;
        if (pair_ok && f2_envelope_pair_supports(log2h, precision) && (!f32_in || (handoff->h_x32_off && handoff->h_x32_off[b] >= 0))) {
            pair_group[log2h - 14].push_back(b);
            ++n_large;
            continue;
        }
        if (log2h > maxl && f2_envelope_split_supports(log2h, precision)) {
            // longer than the LDS-resident transform: four-step transform, all utterances of a size together
            split_groups[log2h].push_back(b);
            ++n_large;
            continue;
        }
        if (log2h > maxl) {
            // beyond that (or float64 transforms): global-memory radix-16 passes, one utterance at a time
            F2_CHECK(ctx, !f32_in, F2_ERR_INVALID, "float32 hand-off is not available for long rows");
            F2_TRY(f2_prof_begin(ctx, F2_K_ENVELOPE));
            F2_TRY(f2_launch_envelope_large(ctx, d_gfb + (size_t)C * (size_t)h_offsets[b],
                                            d_env + (size_t)C * (size_t)h_offsets[b], n, C, P.lpf, P.b0, P.a1, precision));
            F2_TRY(f2_prof_end(ctx, F2_K_ENVELOPE));
            ++n_large;
            continue;
        }
        groups[log2h].push_back(b);
    }
    for (int g = 0; g < 2; ++g)
        if (!pair_group[g].empty())
            F2_TRY(f2_launch_envelope_pair(ctx, d_gfb, d_env, d_offsets, h_offsets, pair_group[g].data(),
                                           (int)pair_group[g].size(), 14 + g, C, P.lpf, P.b0, P.a1,
                                           f32_in ? handoff->d_x32 : nullptr, f32_in ? handoff->d_x32_off : nullptr,
                                           f32_in ? handoff->h_x32_off : nullptr, d_uflag));
    for (int log2h = 0; log2h < 32; ++log2h)
        if (!split_groups[log2h].empty())
            F2_TRY(f2_launch_envelope_split(ctx, d_gfb, d_env, d_offsets, split_groups[log2h].data(),
                                            (int)split_groups[log2h].size(), log2h, C, P.lpf, P.b0, P.a1,
                                            f32_in ? handoff->d_x32 : nullptr, f32_in ? handoff->d_x32_off : nullptr, d_uflag));
    // Utterances of the spectral kernel's length classes that the HOST kept off that route (flag 1 from the start: too little
    // padding for its accuracy guard) are known here: they go first in their group and get one workgroup per row like any
    // envelope launch; the launch that walks the flags with 1 / 16 of the workgroups serves the rest, which only the guard can
    // send back. (All of them behind that launch took 0.9 + 0.5 ms per 2500-utterance launch of the ragged corpus: sixteen rows
    // one after the other on the few workgroups that own an active utterance.)
    std::vector<int> nactive(32, 0);
    bool reordered = false;
    if (d_uflag && h_flag0 && precision == F2_FFT_F32)
        for (int l = F2_SPECTRAL_MIN_LOG2H; l <= 14; ++l) {
            auto& g = groups[l];
            const auto mid = std::stable_partition(g.begin(), g.end(), [&](int b) { return h_flag0[b] != 0; });
            nactive[l] = (int)(mid - g.begin());
            reordered = reordered || (nactive[l] > 0 && nactive[l] < (int)g.size());
        }
    size_t list_elems = 0;
    int ngroups = 0;
    for (auto& g : groups)
        if (!g.empty()) {
            ++ngroups;
            list_elems += g.size();
        }
    const bool identity = ngroups == 1 && (int)list_elems == B && n_large == 0 && !reordered;
    int* d_lists = nullptr;
    if (!identity && ngroups > 0) {
        std::vector<int> flat;
        flat.reserve(list_elems);
        for (auto& g : groups) flat.insert(flat.end(), g.begin(), g.end());
        F2_TRY(f2_reserve(ctx, ctx->work2, sizeof(int) * flat.size()));
        F2_TRY(f2_upload_async(ctx, ctx->work2.ptr, flat.data(), sizeof(int) * flat.size()));
        d_lists = (int*)ctx->work2.ptr;
    }
#ifdef F2_STAMPS
    F2_TRY(f2_stamps_buffer(ctx, (size_t)B * C, 10, &P.stamps));   // (after the pair launcher's report)
#endif
    size_t pos = 0;
    for (int log2h = 0; log2h < 32; ++log2h) {
        const auto& g = groups[log2h];
        if (g.empty()) continue;
        const int* list = identity ? nullptr : d_lists + pos;
        pos += g.size();
        const int nthreads = precision == F2_FFT_F32 ? threads_for<float>(log2h) : threads_for<double>(log2h);
        // one workgroup per row for the utterances ulist[0 .. count)
        auto launch_rows = [&](const int* ulist, size_t count) -> int {
            P.ulist = ulist;
            const dim3 grid((unsigned)(count * (size_t)C)), block(nthreads);
            // the 1 s row without the float low-pass: three-pass plan 16-32-16. Measured against 16-8-4-16: 8 % faster
            // without the low-pass, 6 % with the float64 transform, 4 % slower with the float low-pass
            const bool p3 = log2h == 13 && (!P.lpf || precision == F2_FFT_F64) && !ctx->opt_env_plan4;
            if (precision == F2_FFT_F32) {
                f2_scratch& tw = p3 ? ctx->tw_p3[0] : ctx->tw[0][log2h];
                F2_TRY(ensure_twiddles<float>(ctx, log2h, tw, p3 ? 3 : 4));
                const EnvKernel<float> kern = p3 ? k_envelope<float, 13, 3> : kernel_for<float, MAX_LOG2H_F32>(log2h);
                hipLaunchKernelGGL(kern, grid, block, 0, ctx->stream, P, (const cpx<float>*)tw.ptr);
            } else {
                f2_scratch& tw = p3 ? ctx->tw_p3[1] : ctx->tw[1][log2h];
                F2_TRY(ensure_twiddles<double>(ctx, log2h, tw, p3 ? 3 : 4));
                const EnvKernel<double> kern = p3 ? k_envelope<double, 13, 3> : kernel_for<double, MAX_LOG2H_F64>(log2h);
                hipLaunchKernelGGL(kern, grid, block, 0, ctx->stream, P, (const cpx<double>*)tw.ptr);
            }
            return F2_OK;
        };
        F2_TRY(f2_prof_begin(ctx, F2_K_ENVELOPE));
        if (precision == F2_FFT_F32 && P.uflag && log2h >= F2_SPECTRAL_MIN_LOG2H && log2h <= 14) {
            // a length class the spectral kernel serves: the utterances the host routed here first, one workgroup per row;
            // the others only come here when the guard flags them - walked by far fewer workgroups (f2_envelope_flagged.hip)
            const size_t na = (size_t)nactive[log2h];
            if (na > 0) F2_TRY(launch_rows(list, na));
            if (na < g.size()) {
                P.ulist = list ? list + na : nullptr;
                F2_TRY(f2_launch_envelope_flagged(ctx, P, log2h, (unsigned)(g.size() - na)));
            }
        } else {
            F2_TRY(launch_rows(list, g.size()));
        }
        F2_HIP(ctx, hipGetLastError());
        F2_TRY(f2_prof_end(ctx, F2_K_ENVELOPE));
    }
#ifdef F2_STAMPS
    static const char* names[10] = {"", "load", "fwd fft", "hilbert pairs", "inv fft", "magnitude", "transposed write",
                                    "lpf chunk+scan", "lpf carry+apply", "copy out"};
    F2_TRY(f2_stamps_report(ctx, P.stamps, (size_t)B * C, 10, names, "[stamps]",
                            "mean cycles per workgroup (s_memrealtime, 10 ns ticks):", true));
#endif
    return F2_OK;
}
