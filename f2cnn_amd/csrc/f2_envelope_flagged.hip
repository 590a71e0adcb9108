// K2 for the utterances the spectral kernel's accuracy guard sends back (normally none): k_envelope_flagged walks the
// channels of a flagged utterance with 1 / 16 of the row launch's workgroups. The row itself is the text of
// f2_envelope_row.h, here as the device function envelope_row. Exports only f2_launch_envelope_flagged (f2_internal.h).
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "f2_fft_lds.h"

using namespace f2fft;

namespace {

#define F2_ENVELOPE_ROW_IS_FUNCTION
#include "f2_envelope_row.h"

}  // namespace

int f2_launch_envelope_flagged(f2_ctx* ctx, const f2_env_params& P, int log2h, unsigned nutt) {
    F2_CHECK(ctx, P.uflag && log2h >= F2_SPECTRAL_MIN_LOG2H && log2h <= 14, F2_ERR_INVALID,
             "flagged-row launch outside the spectral kernel's length classes");
    F2_TRY(ensure_twiddles<float>(ctx, log2h, ctx->tw[0][log2h]));
    const cpx<float>* tw = (const cpx<float>*)ctx->tw[0][log2h].ptr;
    const dim3 grid(nutt * ENV_SLICES);
    switch (log2h) {
        case 12: hipLaunchKernelGGL((k_envelope_flagged<float, 12>), grid, dim3(threads_for<float, 12>()), 0, ctx->stream, P, tw); break;
        case 13: hipLaunchKernelGGL((k_envelope_flagged<float, 13>), grid, dim3(threads_for<float, 13>()), 0, ctx->stream, P, tw); break;
        default: hipLaunchKernelGGL((k_envelope_flagged<float, 14>), grid, dim3(threads_for<float, 14>()), 0, ctx->stream, P, tw); break;
    }
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}
