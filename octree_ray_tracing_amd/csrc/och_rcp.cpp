// och_rcp.cpp -- the host's RCPPS and its table model: the capture of this
// CPU's _mm_rcp_ps as a table (host_rcp, och_host_rcp_lut), the model that reads
// a table (och_rcp_from_lut) and a table's error (och_rcp_lut_error).  The only
// unit that needs <immintrin.h>; och_pool.cpp uploads tables (upload_lut).
#include <immintrin.h>

#include <algorithm>
#include <cstdio>
#include <mutex>

#include "och_pool.h"

using och::fail;
using och::host_rcp;
using och::HostRcp;
using och::lut_max_rel_error;

namespace {

inline uint32_t rcpps_native(uint32_t x)
{
    const __m128 r = _mm_rcp_ps(_mm_castsi128_ps(_mm_set1_epi32((int)x)));
    return (uint32_t)_mm_cvtsi128_si32(_mm_castps_si128(r));
}

}  // namespace

namespace och {

const HostRcp &host_rcp()
{
    static HostRcp cap;
    static std::once_flag once;
    std::call_once(once, [] {
        const uint32_t n = 1u << 23;
        std::vector<uint32_t> full(n);
        for (uint32_t m = 0; m < n; m += 4) {
            const __m128i x = _mm_set_epi32((int)(0xBF800000u | (m + 3)), (int)(0xBF800000u | (m + 2)),
                                            (int)(0xBF800000u | (m + 1)), (int)(0xBF800000u | m));
            _mm_storeu_si128((__m128i *)&full[m], _mm_castps_si128(_mm_rcp_ps(_mm_castsi128_ps(x))));
        }
        // Smallest k such that the result only depends on the top k mantissa bits.
        int k = 23;
        for (int cand = 8; cand <= 23; ++cand) {
            const uint32_t block = 1u << (23 - cand);
            bool ok = true;
            for (uint32_t m = 0; m < n && ok; ++m) ok = full[m] == full[m & ~(block - 1)];
            if (ok) { k = cand; break; }
        }
        cap.log2_entries = k;
        cap.lut.resize(1u << k);
        for (uint32_t i = 0; i < (1u << k); ++i) cap.lut[i] = full[(size_t)i << (23 - k)];
        // Check the exponent model on every exponent (negative inputs, as the tracer uses).
        for (uint32_t e = 0; e < 256 && cap.status == OCH_OK; ++e)
            for (uint32_t m = 0; m < n; m += (e == 127 ? 1u : 997u)) {
                const uint32_t x = 0x80000000u | (e << 23) | m;
                if (e == 255 && m) continue;   // NaN payload handling is not used by the tracer
                const uint32_t want = rcpps_native(x);
                const uint32_t got = och_rcp_from_lut(x, cap.lut.data(), k);
                if (want != got) {
                    cap.status = OCH_E_RCP_MODEL;
                    char buf[160];
                    snprintf(buf, sizeof buf, "host RCPPS(0x%08x) = 0x%08x, table model gives 0x%08x", x, want, got);
                    cap.error = buf;
                    break;
                }
            }
    });
    return cap;
}

// Largest relative error |r * x - 1| of the table model over x in [-2, -1):
// entry k serves the mantissa bin [k, k + 1) / 2^L, so the extremes are at
// the bin's ends.  Non-finite or zero entries count as an infinite error.
double lut_max_rel_error(const uint32_t *lut, int log2_entries)
{
    const uint32_t n = 1u << log2_entries;
    double worst = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        float r;
        std::memcpy(&r, &lut[k], 4);
        if (!std::isfinite(r) || r == 0.0F) return INFINITY;
        const double lo = -(1.0 + (double)k / n), hi = -(1.0 + (double)(k + 1) / n);
        worst = std::max({worst, std::fabs((double)r * lo - 1.0), std::fabs((double)r * hi - 1.0)});
    }
    return worst;
}

}  // namespace och

OCH_API uint32_t och_rcp_from_lut(uint32_t x, const uint32_t *lut, int log2_entries)
{
    const uint32_t sign = x & 0x80000000u, e = (x >> 23) & 0xFFu;
    if (e == 0) return sign | 0x7F800000u;
    if (e == 0xFFu) return (x & 0x7FFFFFu) ? (x | 0x400000u) : sign;
    const uint32_t ent = lut[(x & 0x7FFFFFu) >> (23 - log2_entries)];
    const int ne = (int)((ent >> 23) & 0xFFu) + 127 - (int)e;
    return ne <= 0 ? sign : (sign | ((uint32_t)ne << 23) | (ent & 0x7FFFFFu));
}

OCH_API int och_rcp_lut_error(const uint32_t *lut, int log2_entries, double *max_rel_error)
{
    if (!lut || !max_rel_error || log2_entries < 1 || log2_entries > 23) return fail(OCH_E_INVALID, "bad RCPPS table");
    *max_rel_error = lut_max_rel_error(lut, log2_entries);
    return OCH_OK;
}

OCH_API int och_host_rcp_lut(uint32_t *lut, int *log2_entries)
{
    const HostRcp &c = host_rcp();
    if (c.status != OCH_OK) return fail(c.status, "%s", c.error.c_str());
    if (lut) std::memcpy(lut, c.lut.data(), c.lut.size() * sizeof(uint32_t));
    if (log2_entries) *log2_entries = c.log2_entries;
    return OCH_OK;
}
