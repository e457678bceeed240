// aidax_mfmals.hip — k_mfma_ls / k_mfma_ls1 (aidax_mfmals.h): the lone-layer and the three-and-more-layer instantiations, and the host side.
#include "aidax_mfmals.h"

namespace aidax {

static LpFn ls_fn(int hidden, int n_layers, bool chain, int nprod)
{
    if (n_layers == 2) return ls_fn_two_layers(hidden, chain, nprod);
    switch (hidden) {                                       // (a lone layer; deeper stacks: no tiles started below — the same body with M = 0)
#define AIDAX_LS_CASE(HID) case HID: return n_layers == 1 ? ls_fn_for<HID, 1>(chain, nprod) : ls_fn_for<HID, 3>(chain, nprod);
    AIDAX_LS_CASE(16) AIDAX_LS_CASE(32) AIDAX_LS_CASE(48) AIDAX_LS_CASE(64) AIDAX_LS_CASE(80) AIDAX_LS_CASE(96)
#undef AIDAX_LS_CASE
    default: return nullptr;
    }
}
bool mfma_ls_serves(const MfmaDesc& d)
{
    return d.n_layers >= 1 && d.ls_off != 0 && ls_geo(d.n_layers, d.hidden).nw != 0 && ls_fn(d.hidden, d.n_layers, false, 6) != nullptr;
}
size_t mfma_ls_lds_bytes(const MfmaDesc& d, uint32_t n_frames, bool fused)
{
    const size_t body = ls_lds_floats(d.hidden, (int)n_frames, ls_geo(d.n_layers, d.hidden));
    const size_t rows = fused ? (size_t)kMfmaStreams * ((n_frames + 3) & ~3u) + 2 * kChainPackHandFloats : 0;      // lp_chain_rows works in the body's LDS
    return (body > rows ? body : rows) * sizeof(float);
}
bool mfma_ls_fused_serves(const MfmaDesc& d, uint32_t max_frames) { return mfma_ls_serves(d) && max_frames <= (uint32_t)kLpChunk; }
size_t mfma_ls_ring_bytes(const MfmaDesc& d, uint32_t n_streams)
{
    const size_t groups = (n_streams + kMfmaStreams - 1) / kMfmaStreams;
    const LsGeo g = ls_geo(d.n_layers, d.hidden);
    return 256 + groups * (size_t)(d.n_layers - 1) * ls_ring_floats(d.hidden, g.nw, g.m) * sizeof(float);
}
hipError_t launch_mfma_ls_kernel(const LaunchArgs& a, const MfmaDesc& d, float* ring, uint32_t* counters, uint32_t* fault, int n_products,
                                 hipStream_t stream, bool fused)
{
    if (!mfma_ls_serves(d) || a.mode != MODE_CHAIN || (fused && (a.n_frames == 0 || a.n_frames > (uint32_t)kLpChunk))) return hipErrorInvalidValue;
    LpFn fn = ls_fn(d.hidden, d.n_layers, fused, n_products);
    if (!fn || !ring || !counters || !fault) return hipErrorInvalidValue;
    const size_t lds = mfma_ls_lds_bytes(d, a.n_frames, fused);
    if (const hipError_t e = lp_allow_lds(fn, lds); e != hipSuccess) return e;
    const uint32_t groups = (a.n_streams + kMfmaStreams - 1) / kMfmaStreams;
    const uint32_t blocks = d.n_layers == 1 ? groups : ((groups + 7) / 8) * 8 * (uint32_t)d.n_layers;
    return lp_launch(fn, blocks, (uint32_t)(ls_geo(d.n_layers, d.hidden).nw * kWave), lds, stream, a, d, ring, counters, fault);
}

}  // namespace aidax
