// pt_capi_stats.cpp — what pt_get_stats reports: retiring the launch events, the counters, the tables'
// figures, the peers' sums; and pt_stats_reset.
#include "pt_renderer.h"

using namespace pt;

namespace pt {

int collect_pending(pt_renderer* r) {
    if (!r->timing.pending) return PT_OK;
    double sum = 0.0, tsum = 0.0, ssum = 0.0;
    size_t n = 0, tn = 0, sn = 0;
    PT_HIP(r->timing.ev.collect(&sum, &n), "frame events");
    PT_HIP(r->timing.tev.collect(&tsum, &tn), "trace-kernel events");
    double psum = 0.0;
    size_t pn = 0;
    PT_HIP(r->timing.pev.collect(&psum, &pn), "pair-kernel events");
    tsum += psum;  // trace_kernel_* cover k_extend and k_trace_pair together, as before
    tn += pn;
    r->timing.pair_ms += psum;
    r->timing.pair_launches += pn;
    PT_HIP(r->timing.sev.collect(&ssum, &sn), "shading-kernel events");
    r->ahead.spec_pending = false;  // ev.collect waited for every enqueued batch
    r->timing.launches += n;
    r->timing.last_ms = sum;
    r->timing.total_ms += sum;
    r->timing.trace_ms += tsum;
    r->timing.trace_launches += tn;
    r->timing.shade_ms += ssum;
    r->timing.shade_launches += sn;
    r->timing.pending = false;
    return PT_OK;
}

}  // namespace pt

namespace {

// What a multi-device renderer sums over its devices (the times are device 0's).
constexpr uint64_t pt_stats::*kSummed[] = {
    &pt_stats::segments, &pt_stats::samples, &pt_stats::nodes_visited, &pt_stats::tri_tests, &pt_stats::rays,
    &pt_stats::stack_overflows, &pt_stats::wave_steps, &pt_stats::wave_active_lanes, &pt_stats::wave_node_steps,
    &pt_stats::wave_tri_steps, &pt_stats::wave_refills, &pt_stats::lds_nodes_visited, &pt_stats::shade_kernel_items,
    &pt_stats::shadow_rays, &pt_stats::trace_kernel_rays, &pt_stats::trace_kernel_bytes, &pt_stats::strict_retraces,
    &pt_stats::nee_unoccluded,
    // the per-kernel ray and byte counts of every device, like trace_kernel_*
    &pt_stats::pair_kernel_rays, &pt_stats::pair_kernel_bytes, &pt_stats::pair_kernel_shadow_rays,
    &pt_stats::lit_table_answers, &pt_stats::occluder_table_answers, &pt_stats::skip_table_rays,
    &pt_stats::queue_bytes};

// The lit and occluder tables' figures; the caller has synchronised, so the last builds' events
// are done.
int table_stats(pt_renderer* r, pt_stats* out) {
    r->lit.built.harvest();
    // the table's own figures only while it is in use: wanted for the renderer's state and built for its lights
    if (lit_wanted(r) && table_current(r, r->lit.built)) {
        const size_t nw = (size_t)r->lit.words * (size_t)r->lit.built.n;
        if (r->lit.built.count < 0) {
            std::vector<uint32_t> hb(nw);
            PT_HIP(hipMemcpy(hb.data(), r->lit.d_bits, sizeof(uint32_t) * nw, hipMemcpyDeviceToHost),
                   "download lit table");
            int64_t n = 0;
            for (uint32_t w : hb) n += __builtin_popcount(w);
            r->lit.built.count = n;
        }
        out->lit_table_cells = r->lit.cells;
        out->lit_table_bits_set = (uint64_t)r->lit.built.count;
        out->lit_table_bytes = sizeof(uint32_t) * ((size_t)r->ntri + (size_t)r->lit.words * kLitMaxLights);
        out->lit_table_build_ms = r->lit.built.build_ms;
    }
    r->occ.built.harvest();
    // like the lit fields: only while the table is in use and built for the renderer's lights
    if (occ_wanted(r) && r->occ.d_tab && table_current(r, r->occ.built)) {
        const size_t ne = (size_t)r->lit.cells * (size_t)r->occ.built.n;
        if (r->occ.built.count < 0) {
            std::vector<int> ho(ne);
            PT_HIP(hipMemcpy(ho.data(), r->occ.d_tab, sizeof(int) * ne, hipMemcpyDeviceToHost), "download occluder table");
            int64_t n = 0;
            for (int t : ho) n += t >= 0;
            r->occ.built.count = n;
        }
        out->occluder_table_bytes = sizeof(int) * ne;
        out->occluder_table_candidates = (uint64_t)r->occ.built.count;
        out->occluder_table_build_ms = r->occ.built.build_ms;
    }
    r->skip.built.harvest();
    if (skip_wanted(r) && r->skip.d_words && r->skip.built.current(r->skip.version, nullptr, 0)) {
        out->skip_table_bytes = sizeof(uint32_t) * 2 * (size_t)r->ntri;
        out->skip_table_build_ms = r->skip.built.build_ms;
    }
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_get_stats(pt_renderer* r, pt_stats* out) {
    if (!r || !out) return fail(PT_ERR_INVALID, "pt_get_stats: NULL");
    int rc = pt_synchronize(r);
    if (rc) return rc;
    unsigned long long c[kCounters];
    PT_HIP(hipMemcpy(c, r->d_counters, sizeof c, hipMemcpyDeviceToHost), "download counters");
    std::memset(out, 0, sizeof *out);
    out->segments = c[kCtrSegments];
    out->samples = r->timing.samples;
    out->last_render_ms = r->timing.last_ms;
    out->total_render_ms = r->timing.total_ms;
    out->render_calls = r->timing.calls;
    out->kernel_launches = r->timing.launches;
    out->frames_per_launch = r->frames_per_launch;
    out->bvh_build_ms = r->timing.bvh_ms;
    out->bvh_nodes = r->bvh_nodes;
    out->bvh_depth = r->bvh_depth;
    out->nodes_visited = c[kCtrNodes];
    out->tri_tests = c[kCtrTriTests];
    out->rays = c[kCtrRays];
    out->stack_overflows = c[kCtrStackOverflows];
    out->triangles = r->ntri;
    out->trace_kernel_ms = r->timing.trace_ms;
    out->trace_kernel_launches = r->timing.trace_launches;
    out->pair_kernel_ms = r->timing.pair_ms;
    out->pair_kernel_launches = r->timing.pair_launches;
    out->shadow_rays = c[kCtrShadowRays];
    out->trace_kernel_rays = c[kCtrTraceRays];
    out->trace_kernel_bytes = c[kCtrTraceBytes];
    out->strict_retraces = 0;  // no traversal re-traces any more (pt_device.h tri_accept_in); ABI field
    out->wave_steps = c[kCtrWaveSteps];
    out->wave_active_lanes = c[kCtrWaveActive];
    out->wave_node_steps = c[kCtrWaveNodeSteps];
    out->wave_tri_steps = c[kCtrWaveTriSteps];
    out->wave_refills = c[kCtrWaveRefills];
    out->lds_nodes_visited = c[kCtrLdsNodes];
    out->shade_kernel_ms = r->timing.shade_ms;
    out->shade_kernel_launches = r->timing.shade_launches;
    out->shade_kernel_items = c[kCtrShadeItems];
    out->frames_rendered_ahead = r->ahead.rendered;
    out->frames_served_ahead = r->ahead.served;
    out->look_ahead_cancelled = r->ahead.cancelled;
    out->pair_kernel_rays = c[kCtrPairRays];
    out->pair_kernel_bytes = c[kCtrPairBytes];
    out->pair_kernel_shadow_rays = c[kCtrPairShadowRays];
    out->nee_unoccluded = c[kCtrNeeUnoccluded];
    out->queue_bytes = queue_bytes_held(r);
    const size_t qb = queue_budget_bytes(r);
    out->queue_budget = qb == SIZE_MAX ? 0 : qb;
    out->last_streams = r->last_streams;
    out->last_batch_frames = r->last_batch;
    out->look_ahead_held = r->ahead.held;
    out->lit_table_answers = c[kCtrLitAnswers];
    out->occluder_table_answers = c[kCtrOccAnswers];
    out->skip_table_rays = c[kCtrSkipRays];
    if ((rc = table_stats(r, out)) != PT_OK) return rc;
    out->geometry_commits = r->geom.commits;
    out->geometry_refits = r->geom.refits;
    out->geometry_rebuilds = r->geom.rebuilds;
    out->geometry_commit_ms = r->geom.commit_ms;
    out->bvh_sah_cost = r->geom.sah_cost;
    out->bvh_sah_cost_built = r->geom.sah_cost_built;
    // a multi-device renderer reports the work of all its devices (times are device 0's)
    for (pt_renderer* p : r->multi.peers) {
        pt_stats ps;
        rc = pt_get_stats(p, &ps);
        if (rc) return rc;
        for (uint64_t pt_stats::*f : kSummed) out->*f += ps.*f;
    }
    return PT_OK;
}

int pt_stats_reset(pt_renderer* r) {
    if (!r) return fail(PT_ERR_INVALID, "pt_stats_reset: NULL");
    int rc = pt_synchronize(r);
    if (rc) return rc;
    for (pt_renderer* p : r->multi.peers) {
        if ((rc = pt_stats_reset(p)) != PT_OK) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipMemset(r->d_counters, 0, kCounters * sizeof(unsigned long long)), "hipMemset counters");
    r->timing.reset_counts();
    r->ahead.reset_counts();
    return PT_OK;
}

}  // extern "C"
