// pt_capi_tables.cpp — the lit table, the occluder candidate table and the skip table: when they are
// wanted, built and current, and the bodies of their download and upload calls.
#include "pt_renderer.h"
#include "pt_skip.h"

using namespace pt;

namespace pt {

// BuiltTable (pt_renderer.h): the state both tables keep about their last build.
int BuiltTable::begin(hipStream_t stream) {
    PT_HIP(ev[0].ensure(), "hipEventCreate");
    PT_HIP(ev[1].ensure(), "hipEventCreate");
    PT_HIP(hipEventRecord(ev[0], stream), "hipEventRecord");
    return PT_OK;
}
int BuiltTable::end(hipStream_t stream, uint32_t v, const void* l, int nl) {
    PT_HIP(hipEventRecord(ev[1], stream), "hipEventRecord");
    ev_pending = true;
    count = -1;
    version = v;
    lights = l;
    n = nl;
    return PT_OK;
}
void BuiltTable::harvest() {
    if (!ev_pending) return;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
        build_ms = ms;
    else
        (void)hipGetLastError();
    ev_pending = false;
}
// Whether table t was built for the renderer's lights as they are now.
bool table_current(const pt_renderer* r, const BuiltTable& t) {
    return t.current(r->lit.version, r->d_lights, r->n_lights);
}

// The lit table for this call's lights (pt_lit.h): decides whether the call's launches use it
// (r->lit.active) and rebuilds the bits when they are stale.  The build runs on r->stream, which
// every earlier batch has joined (launch_frames), so batches already enqueued keep the bits they
// were enqueued with until they are done, and the batches enqueued next see the new ones.
#ifndef PT_LIT_TABLE
#define PT_LIT_TABLE 1  // auto (pt_set_lit_table < 0): 1 = on where it pays, 0 = off (A/B builds)
#endif
bool lit_wanted(const pt_renderer* r) {
    // auto: on in the modes where three interleaved runs per side cleared three times the parent's
    // spread at 1080p (Lambert +6.8 %, Default +1.9 %, Layered +1.6 %); Dielectric lost 1.2 % (its
    // register-bound k_shade_fused spills more) and Conductor is not measured
    const bool pays = r->material_mode == PT_MAT_LAMBERT || r->material_mode == PT_MAT_DEFAULT ||
                      r->material_mode == PT_MAT_LAYERED;
    // A pt_launch call carries its own device light array, whose contents the host cannot compare
    // with the built ones, and renders one frame, which cannot pay for a build (2 ms on the sphere
    // box, about a 1080p frame): auto neither uses nor rebuilds the table there, and the table of the
    // renderer's own lights stays valid.  pt_set_lit_table(1) rebuilds it for every such call.
    const bool on = r->lit.mode < 0 ? PT_LIT_TABLE != 0 && pays && !r->lit.launch_call : r->lit.mode > 0;
    return on && r->lit.d_tri && r->d_lights && r->n_lights >= 1 && r->n_lights <= kLitMaxLights;
}
// The occluder candidate table (pt_lit.hip k_occ_build) rides on the lit table: same cells, same
// lights, rebuilt right after the bits on the same stream.
#ifndef PT_OCC_TABLE
#define PT_OCC_TABLE 1  // auto (pt_set_occluder_table < 0): 1 = on where it pays, 0 = off (A/B builds)
#endif
bool occ_wanted(const pt_renderer* r) {
    // the kernels that carry the test: k_shade_fused<Lambert> and k_shade_a (Default, Layered); it is
    // compiled out of the Conductor and Dielectric kernels, which would build the table for nothing
    const bool has_code = r->material_mode == PT_MAT_LAMBERT || r->material_mode == PT_MAT_DEFAULT ||
                          r->material_mode == PT_MAT_LAYERED;
    // auto: on in all three -- three interleaved runs per side at 1080p, the slowest run with the table
    // above the parent's fastest by more than three parent spreads: Lambert +4.8 %, Default +1.3 %
    // (sphere box; one of its two sets of runs had a noisier parent and missed the bar) and +1.7 %
    // (atrium), Layered +1.0 %; the textured atrium (Default) neither gains nor loses
    const bool pays = has_code;
    // auto follows the lit table's auto only: a caller who forces the lit table on is measuring that
    // table by itself (one traced ray less per lit answer) and asks for the candidates explicitly
    const bool on = r->occ.mode < 0 ? PT_OCC_TABLE != 0 && pays && r->lit.mode < 0 : r->occ.mode > 0;
    return on && has_code && !r->occ.alloc_failed && lit_wanted(r);
}
// After the lit bits are current on r->stream (lit_prepare): the candidates for the same lights.
static int occ_prepare(pt_renderer* r) {
    r->occ.active = occ_wanted(r);
    if (!r->occ.active) return PT_OK;
    if (table_current(r, r->occ.built)) return PT_OK;
    const size_t need = (size_t)r->lit.cells * (size_t)r->n_lights;
    // hipFree waits for the batches that still read the old array
    if (need > r->occ.d_tab.size() && r->occ.d_tab.alloc(need) != hipSuccess) {  // not an error: no table
        r->occ.alloc_failed = true;
        r->occ.active = false;
        return PT_OK;
    }
    int rc = r->occ.built.begin(r->stream);
    if (rc != PT_OK) return rc;
    PT_HIP(occ_build(r->scene(), r->lit.d_tri, r->lit.cells, r->lit.words, r->d_lights, r->n_lights, r->lit.d_bits,
                     r->occ.d_tab, r->stream),
           "occ_build");
    return r->occ.built.end(r->stream, r->lit.version, r->d_lights, r->n_lights);
}
int lit_prepare(pt_renderer* r) {
    r->lit.active = lit_wanted(r);
    r->occ.active = false;
    if (!r->lit.active) return PT_OK;
    if (table_current(r, r->lit.built)) return occ_prepare(r);
    int rc = r->lit.built.begin(r->stream);
    if (rc != PT_OK) return rc;
    PT_HIP(lit_build(r->scene(), r->lit.d_tri, r->lit.cells, r->lit.words, r->d_lights, r->n_lights, r->lit.d_bits,
                     r->lit.diag, r->stream),
           "lit_build");
    if ((rc = r->lit.built.end(r->stream, r->lit.version, r->d_lights, r->n_lights)) != PT_OK) return rc;
    return occ_prepare(r);
}

// The skip table (pt_skip.h): extension rays drop one proven-unhittable BVH subtree each.
#ifndef PT_SKIP_TABLE
#define PT_SKIP_TABLE 1  // auto (pt_set_skip_table < 0): 1 = on where it pays, 0 = off (A/B builds)
#endif
bool skip_wanted(const pt_renderer* r) {
    // the kernels that carry the lookup and the compare: k_shade_fused / k_shade0_pixel and
    // k_trace_pair of the three fused modes
    const bool has_code = r->material_mode == PT_MAT_LAMBERT || r->material_mode == PT_MAT_CONDUCTOR ||
                          r->material_mode == PT_MAT_DIELECTRIC;
    // auto: Lambert, where three interleaved runs per side at 1080p cleared three parent spreads (+8 %,
    // DESIGN.md §5 v62); Conductor and Dielectric are not measured with the table on
    const bool pays = r->material_mode == PT_MAT_LAMBERT;
    const bool on = r->skip.mode < 0 ? PT_SKIP_TABLE != 0 && pays : r->skip.mode > 0;
    return on && has_code && r->skip.in_bounds && !r->skip.alloc_failed && r->ntri > 0 && r->bvh_nodes > 0;
}
// Decides whether the next launches use the table (r->skip.active) and rebuilds the words on r->stream
// when the records or the tree have changed since the last build.  Like the lit bits, the build runs
// on the stream every earlier batch has joined, so batches in flight keep the words they started with.
int skip_prepare(pt_renderer* r) {
    r->skip.active = skip_wanted(r);
    if (!r->skip.active) return PT_OK;
    if (r->skip.built.current(r->skip.version, nullptr, 0)) return PT_OK;
    const size_t ntri = (size_t)r->ntri, nn = (size_t)r->bvh_nodes + 1;  // + the scene's sliver flag
    // hipFree waits for the batches that still read the old arrays
    if ((2 * ntri > r->skip.d_words.size() && r->skip.d_words.alloc(2 * ntri) != hipSuccess) ||
        (nn > r->skip.d_node_parent.size() && r->skip.d_node_parent.alloc(nn) != hipSuccess) ||
        (ntri > r->skip.d_tri_parent.size() && r->skip.d_tri_parent.alloc(ntri) != hipSuccess)) {
        (void)hipGetLastError();  // not an error: no table
        r->skip.alloc_failed = true;
        r->skip.active = false;
        return PT_OK;
    }
    int rc = r->skip.built.begin(r->stream);
    if (rc != PT_OK) return rc;
    PT_HIP(skip_build(r->scene(), r->skip.d_node_parent, r->skip.d_tri_parent, r->skip.d_words, r->stream), "skip_build");
    return r->skip.built.end(r->stream, r->skip.version, nullptr, 0);
}

int skip_table_download(pt_renderer* r, int64_t* words_out, uint32_t* words, int64_t bytes) {
    int rc = skip_prepare(r);
    if (rc) return rc;
    *words_out = r->skip.active ? 2 * (int64_t)r->ntri : 0;
    if (!r->skip.active || !words) return PT_OK;
    if (bytes != (int64_t)sizeof(uint32_t) * *words_out) return fail(PT_ERR_INVALID, "pt_skip_table_download: size mismatch");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    PT_HIP(hipMemcpy(words, r->skip.d_words, (size_t)bytes, hipMemcpyDeviceToHost), "download skip table");
    return PT_OK;
}

// The lit table's cells for the leaf-ordered records in force (pt_create, and every geometry
// commit): lit_subdivide on a host copy; a scene outside the table's limits runs without it until
// a later commit brings it back inside.  The bits are stale either way (lit.version).
int lit_resubdivide(pt_renderer* r) {
    const size_t ntri = (size_t)r->ntri;
    std::vector<float4> isect_host(3 * ntri);
    PT_HIP(hipMemcpy(isect_host.data(), r->d_isect, sizeof(float4) * 3 * ntri, hipMemcpyDeviceToHost), "download isect");
    std::vector<uint32_t> lit_words_host;
    uint32_t cells = 0;
    float diag = 0.0f;
    r->lit.version++;
    r->lit.built.invalidate_count();
    // the skip table follows the same records (and the tree they were built or refitted into)
    r->skip.version++;
    r->skip.alloc_failed = false;
    r->skip.in_bounds = true;
    for (size_t t = 0; t < ntri && r->skip.in_bounds; ++t)
        r->skip.in_bounds = skip_tri_in_bounds(reinterpret_cast<const float*>(isect_host.data()), (int)t);
    if (!lit_subdivide(isect_host.data(), (int)ntri, lit_words_host, &cells, &diag)) {
        r->lit.d_tri.reset();  // lit_wanted: no table
        r->lit.cells = r->lit.words = 0;
        return PT_OK;
    }
    const uint32_t words = (cells + 31) / 32;
    hipError_t e = hipSuccess;
    if (words > r->lit.words_cap) {
        e = r->lit.d_bits.alloc((size_t)words * kLitMaxLights);
        r->lit.words_cap = e == hipSuccess ? words : 0;
    }
    if (e == hipSuccess && !r->lit.d_tri) e = r->lit.d_tri.alloc(ntri);
    if (e == hipSuccess)
        e = hipMemcpy(r->lit.d_tri, lit_words_host.data(), sizeof(uint32_t) * ntri, hipMemcpyHostToDevice);
    if (e != hipSuccess) {  // no table rather than a stale one
        r->lit.d_tri.reset();
        r->lit.cells = r->lit.words = 0;
        return hip_fail(e, "lit table");
    }
    r->lit.cells = cells;
    r->lit.words = words;
    r->lit.diag = diag;
    r->occ.alloc_failed = false;  // occ_prepare sizes the candidates' array for the new cells
    return PT_OK;
}

int lit_table_download(pt_renderer* r, pt_lit_table_info* info, uint32_t* tri_words, int64_t tri_bytes, uint32_t* bits,
                       int64_t bits_bytes) {
    int rc = lit_prepare(r);
    if (rc) return rc;
    std::memset(info, 0, sizeof *info);
    info->active = r->lit.active ? 1 : 0;
    info->delta = kLitDelta;
    if (!r->lit.active) return PT_OK;
    info->lights = r->n_lights;
    info->triangles = (uint32_t)r->ntri;
    info->cells = r->lit.cells;
    info->words_per_light = r->lit.words;
    info->margin = lit_margin(r->lit.diag);  // the upper bound of the cells' margins (lit_margin_cell)
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    if (tri_words) {
        if (tri_bytes != (int64_t)(sizeof(uint32_t) * (size_t)r->ntri))
            return fail(PT_ERR_INVALID, "pt_lit_table_download: tri_words size mismatch");
        PT_HIP(hipMemcpy(tri_words, r->lit.d_tri, (size_t)tri_bytes, hipMemcpyDeviceToHost), "download lit table");
    }
    if (bits) {
        if (bits_bytes != (int64_t)(sizeof(uint32_t) * (size_t)r->lit.words * (size_t)r->n_lights))
            return fail(PT_ERR_INVALID, "pt_lit_table_download: bits size mismatch");
        PT_HIP(hipMemcpy(bits, r->lit.d_bits, (size_t)bits_bytes, hipMemcpyDeviceToHost), "download lit table");
    }
    return PT_OK;
}

int occ_table_download(pt_renderer* r, int64_t* entries_out, int32_t* entries, int64_t bytes) {
    int rc = lit_prepare(r);
    if (rc) return rc;
    *entries_out = r->occ.active ? (int64_t)r->lit.cells * (int64_t)r->n_lights : 0;
    if (!r->occ.active || !entries) return PT_OK;
    if (bytes != (int64_t)sizeof(int32_t) * *entries_out)
        return fail(PT_ERR_INVALID, "pt_occluder_table_download: size mismatch");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    PT_HIP(hipMemcpy(entries, r->occ.d_tab, (size_t)bytes, hipMemcpyDeviceToHost), "download occluder table");
    return PT_OK;
}

int occ_table_upload(pt_renderer* r, const int32_t* entries, int64_t bytes) {
    int rc = pt_synchronize(r);  // no batch in flight reads the entries while they change
    if (rc) return rc;
    if ((rc = lit_prepare(r)) != PT_OK) return rc;
    if (!r->occ.active) return fail(PT_ERR_INVALID, "pt_occluder_table_upload: the table is not in use");
    const int64_t n = (int64_t)r->lit.cells * (int64_t)r->n_lights;
    if (bytes != (int64_t)sizeof(int32_t) * n) return fail(PT_ERR_INVALID, "pt_occluder_table_upload: size mismatch");
    for (int64_t i = 0; i < n; ++i)
        if (entries[i] < -1 || entries[i] >= r->ntri)
            return fail(PT_ERR_INVALID, "pt_occluder_table_upload: entry out of range");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");  // the build above, if any
    PT_HIP(hipMemcpy(r->occ.d_tab, entries, (size_t)bytes, hipMemcpyHostToDevice), "upload occluder table");
    r->occ.built.invalidate_count();
    return PT_OK;
}

}  // namespace pt
