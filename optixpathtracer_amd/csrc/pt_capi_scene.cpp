// pt_capi_scene.cpp — everything between a pt_scene and a tree in force: upload, BVH build, SAH cost,
// geometry commits.
#include "pt_renderer.h"

using namespace pt;

namespace {

// A mesh whose normals stay in object space (pt_device.h kNormalObject) needs the kernels'
// TEX instantiations, which S.texinfo selects: an untextured scene gets a one-entry array that no
// record refers to.
int need_tex_kernels(pt_renderer* r) {
    if (r->d_texinfo) return PT_OK;
    bool any = false;
    for (int m = 0; m < r->nmesh; ++m) any = any || r->geom.host.normal_mode(m) == 2;
    if (!any) return PT_OK;
    PT_HIP(r->d_texinfo.alloc(1), "hipMalloc texinfo");
    PT_HIP(hipMemset(r->d_texinfo, 0, sizeof(int4)), "hipMemset texinfo");
    return PT_OK;
}

// Upload the baked soup and build the BVH4 and the leaf-ordered records into `bo`'s buffers with the
// renderer's builder; *ms (optional) = device time of the build.  Synchronises the library stream.
int build_tree(pt_renderer* r, const std::vector<float4>& tri, const std::vector<float4>& nrm, const float cmin[3],
               const float cmax[3], BuildOutput& bo, float* ms_out = nullptr) {
    const size_t ntri = tri.size() / 3;
    DevBuf<float4> d_uv_orig, d_nrm_orig, d_tri_orig;  // released at return, after the wait below
    hipError_t e = d_tri_orig.alloc(3 * ntri);
    if (e == hipSuccess) e = d_nrm_orig.alloc(3 * ntri);
    if (e == hipSuccess && bo.tuv) e = d_uv_orig.alloc(2 * ntri);
    if (e == hipSuccess && bo.tuv)
        e = hipMemcpyAsync(d_uv_orig, r->geom.host.uvs.data(), sizeof(float4) * 2 * ntri, hipMemcpyHostToDevice,
                           r->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_tri_orig, tri.data(), sizeof(float4) * 3 * ntri, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_nrm_orig, nrm.data(), sizeof(float4) * 3 * ntri, hipMemcpyHostToDevice, r->stream);
    float ms = 0.0f;
    if (e == hipSuccess) {
        BuildInput in;
        in.tri_orig = d_tri_orig;
        in.nrm_orig = d_nrm_orig;
        in.uv_orig = d_uv_orig;
        in.n = (int)ntri;
        // AUTO: the binned-SAH tree (fewest node visits of the builders), built on the
        // GPU; every peer of a multi-device renderer builds its own on its own device
        in.builder = r->geom.builder;
        in.tri_host = tri.data();
        for (int a = 0; a < 3; ++a) {
            in.cmin[a] = cmin[a];
            in.cmax[a] = cmax[a];
        }
        e = bvh_build(in, bo, r->stream, &ms);
    }
    (void)hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return hip_fail(e, "bvh_build");
    if (ms_out) *ms_out = ms;
    else r->timing.bvh_ms = ms;
    return PT_OK;
}

// The SAH cost of the BVH4 in force -> r->geom.sah_cost (pt_stats bvh_sah_cost): the sum over every node
// and leaf of its stored box's half area times kSahCNode (a node, the root included) or kSahCTri x
// triangles (a leaf), in fp64 -- per-block partials (k_sah_partial) added here in block order --
// over the half area the root had when the tree was last built.  `built`: the tree was just
// built, so that root is this one and bvh_sah_cost_built takes the same value.  `after` (optional)
// is recorded behind the kernel.  Synchronises the library stream.
int sah_cost_now(pt_renderer* r, bool built, hipEvent_t after = nullptr) {
    const int nb = sah_partial_blocks(r->bvh_nodes);
    std::vector<double> part((size_t)nb + 1, 0.0);
    if (nb > 0) PT_HIP(sah_partial_launch(r->d_nodes, r->bvh_nodes, r->geom.d_sah_part, r->stream), "k_sah_partial");
    if (after) PT_HIP(hipEventRecord(after, r->stream), "hipEventRecord");
    if (nb > 0)
        PT_HIP(hipMemcpyAsync(part.data(), r->geom.d_sah_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost,
                              r->stream),
               "download SAH partials");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    double sum = 0.0;
    for (int b = 0; b < nb; ++b) sum += part[(size_t)b];
    if (built) r->geom.sah_root_built = part[(size_t)nb];
    r->geom.sah_cost = r->geom.sah_root_built > 0.0 ? sum / r->geom.sah_root_built : 0.0;
    if (built) r->geom.sah_cost_built = r->geom.sah_cost;
    return PT_OK;
}

// staged -> retained host copy; the dirty meshes' records for k_rebake
int apply_staged(pt_renderer* r, std::vector<RefitMesh>& rm) {
    GeomHost& G = r->geom.host;
    for (int m = 0; m < r->nmesh; ++m) {
        StagedMesh& sm = r->geom.staged[(size_t)m];
        const size_t v0 = (size_t)G.voff[(size_t)m], nv = (size_t)G.voff[(size_t)m + 1] - v0;
        if (sm.has_model) std::memcpy(&G.model[16 * (size_t)m], sm.model, sizeof sm.model);
        for (size_t v = 0; sm.has_verts && v < nv; ++v)
            G.verts[v0 + v] = make_float4(sm.verts[3 * v], sm.verts[3 * v + 1], sm.verts[3 * v + 2], 0.0f);
        for (size_t v = 0; sm.has_norms && v < nv; ++v)
            G.norms[v0 + v] = make_float4(sm.norms[3 * v], sm.norms[3 * v + 1], sm.norms[3 * v + 2], 0.0f);
        RefitMesh& d = rm[(size_t)m];
        std::memcpy(d.m, &G.model[16 * (size_t)m], sizeof d.m);
        d.dirty = (sm.has_model || sm.has_verts) ? 1 : 0;
        d.normal_mode = G.normal_mode(m);
        if (sm.has_model) G.normal_rows(m, &r->geom.mats[(size_t)kMatStride * (size_t)m]);
        d.pad[0] = d.pad[1] = 0;
        if (r->ntri > 0 && nv > 0 && sm.has_verts)
            PT_HIP(hipMemcpy(r->geom.d_overts + v0, &G.verts[v0], sizeof(float4) * nv, hipMemcpyHostToDevice),
                   "upload vertices");
        if (r->ntri > 0 && nv > 0 && sm.has_norms)
            PT_HIP(hipMemcpy(r->geom.d_onorms + v0, &G.norms[v0], sizeof(float4) * nv, hipMemcpyHostToDevice),
                   "upload normals");
        sm = StagedMesh();
    }
    return PT_OK;
}

// rebuild: the create path's bake and build into temporary buffers, swapped in on success (the
// old ones, or the unused new ones, are released at return); on failure the refitted tree stays in force
int rebuild_tree(pt_renderer* r) {
    const size_t ntri = (size_t)r->ntri;
    std::vector<float4> tri, nrm;
    float cmin[3], cmax[3];
    bake_scene(r->geom.host, tri, nrm, cmin, cmax);
    DevBuf<float4> tuv, shade, isect;
    DevBuf<BNode4> nodes;
    hipError_t e = nodes.alloc(std::max<size_t>(1, ntri));
    if (e == hipSuccess) e = isect.alloc(3 * ntri);
    if (e == hipSuccess) e = shade.alloc(4 * ntri);
    if (e == hipSuccess && r->d_tuv) e = tuv.alloc(2 * ntri);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc rebuild buffers");
    BuildOutput bo;
    bo.nodes = nodes;
    bo.isect = isect;
    bo.shade = shade;
    bo.tuv = tuv;
    float bms = 0.0f;
    const int rc = build_tree(r, tri, nrm, cmin, cmax, bo, &bms);
    if (rc != PT_OK) return rc;
    if (3 * bo.depth > kMinTraversalStack)
        return fail(PT_ERR_INVALID, "pt_commit_geometry: the rebuilt BVH is too deep for the traversal stack (depth " +
                                        std::to_string(bo.depth) + "); the refitted tree stays in force");
    r->d_nodes.swap(nodes);
    r->d_isect.swap(isect);
    r->d_shade.swap(shade);
    r->d_tuv.swap(tuv);
    r->bvh_nodes = bo.n_nodes;
    r->bvh_depth = bo.depth;
    r->geom.level_base = bo.level_base;
    r->geom.commit_ms += bms;
    return PT_OK;
}

}  // namespace

namespace pt {

// The first device half of pt_create: the renderer's streams and counters, the material records and
// the textures.  r->geom.mats holds the records already.
int upload_scene(pt_renderer* r, const pt_scene* scene, const std::vector<int4>& texinfo, size_t ntexel) {
    const std::vector<float4>& mats = r->geom.mats;
    const int ntex = scene->n_textures;
    PT_HIP(r->stream.create(), "hipStreamCreate");
    // The download stream and the second wavefront stream right after the library stream: HIP
    // spreads streams over GPU_MAX_HW_QUEUES (4) hardware queues in creation order, and two streams
    // that land on one queue run in sequence.  Created lazily (first pt_render, first two-batch
    // render) they could share a queue with r->stream after other streams had been created in
    // between; then a pt_render download waited for the look-ahead batch behind it on that queue.
    PT_HIP(r->dl_stream.create(), "hipStreamCreate");
    PT_HIP(r->xstream[1].create(), "hipStreamCreate");
    PT_HIP(r->ev_join[1].ensure(hipEventDisableTiming), "hipEventCreate");
    PT_HIP(r->d_counters.alloc(kCounters), "hipMalloc counters");
    PT_HIP(hipMemsetAsync(r->d_counters, 0, kCounters * sizeof(unsigned long long), r->stream), "hipMemset");
    PT_HIP(r->d_mats.alloc(mats.size()), "hipMalloc mats");
    PT_HIP(hipMemcpyAsync(r->d_mats, mats.data(), sizeof(float4) * mats.size(), hipMemcpyHostToDevice, r->stream),
           "upload mats");
    if (ntex > 0) {
        PT_HIP(r->d_texinfo.alloc((size_t)ntex), "hipMalloc texinfo");
        PT_HIP(hipMemcpyAsync(r->d_texinfo, texinfo.data(), sizeof(int4) * (size_t)ntex, hipMemcpyHostToDevice,
                              r->stream),
               "upload texinfo");
        PT_HIP(r->d_texels.alloc(ntexel), "hipMalloc texels");
        for (int k = 0; k < ntex; ++k) {
            const pt_texture& tx = scene->textures[k];
            PT_HIP(hipMemcpy(r->d_texels + texinfo[(size_t)k].x, tx.rgba8,
                             sizeof(uint32_t) * (size_t)tx.width * (size_t)tx.height, hipMemcpyHostToDevice),
                   "upload texels");
        }
    }
    return need_tex_kernels(r);
}

// The second: the bake of the retained scene, the tree, the retained scene on the device for the
// geometry updates, the SAH cost and the lit table's cells.  Waits for the library stream.
int build_scene(pt_renderer* r, bool any_tex) {
    const size_t ntri = (size_t)r->ntri;
    if (ntri > 0) {
        std::vector<float4> tri, nrm;
        float cmin[3], cmax[3];
        bake_scene(r->geom.host, tri, nrm, cmin, cmax);
        if (any_tex) PT_HIP(r->d_tuv.alloc(2 * ntri), "hipMalloc tuv");
        PT_HIP(r->d_isect.alloc(3 * ntri), "hipMalloc isect");
        PT_HIP(r->d_shade.alloc(4 * ntri), "hipMalloc shade");
        PT_HIP(r->d_nodes.alloc(std::max<size_t>(1, ntri)), "hipMalloc nodes");
        BuildOutput bo;
        bo.nodes = r->d_nodes;
        bo.isect = r->d_isect;
        bo.shade = r->d_shade;
        bo.tuv = r->d_tuv;
        int rc = build_tree(r, tri, nrm, cmin, cmax, bo);
        if (rc != PT_OK) return rc;
        r->bvh_nodes = bo.n_nodes;
        r->bvh_depth = bo.depth;
        r->geom.level_base = bo.level_base;
        // a traversal holds at most 3 stack entries per BVH4 level; the smallest traversal stack
        // (kMinTraversalStack) must hold them, or rays could lose subtrees
        if (3 * bo.depth > kMinTraversalStack)
            return fail(PT_ERR_INVALID, "pt_create: BVH too deep for the traversal stack (depth " +
                                            std::to_string(bo.depth) + ")");
        // retained on the device for k_rebake, and the SAH cost of the tree as built
        const size_t nv = r->geom.host.verts.size();
        PT_HIP(r->geom.d_overts.alloc(std::max<size_t>(1, nv)), "hipMalloc vertices");
        PT_HIP(r->geom.d_onorms.alloc(std::max<size_t>(1, nv)), "hipMalloc normals");
        PT_HIP(r->geom.d_tidx.alloc(ntri), "hipMalloc indices");
        PT_HIP(r->geom.d_rmesh.alloc((size_t)std::max(1, r->nmesh)), "hipMalloc mesh records");
        PT_HIP(r->geom.d_sah_part.alloc((size_t)sah_partial_blocks((int)ntri) + 1), "hipMalloc SAH partials");
        PT_HIP(r->geom.ev[0].ensure(), "hipEventCreate");
        PT_HIP(r->geom.ev[1].ensure(), "hipEventCreate");
        if (nv > 0) {
            PT_HIP(hipMemcpy(r->geom.d_overts, r->geom.host.verts.data(), sizeof(float4) * nv, hipMemcpyHostToDevice),
                   "upload vertices");
            PT_HIP(hipMemcpy(r->geom.d_onorms, r->geom.host.norms.data(), sizeof(float4) * nv, hipMemcpyHostToDevice),
                   "upload normals");
        }
        PT_HIP(hipMemcpy(r->geom.d_tidx, r->geom.host.tidx.data(), sizeof(int4) * ntri, hipMemcpyHostToDevice),
               "upload indices");
        if ((rc = sah_cost_now(r, true)) != PT_OK) return rc;
        // lit table: the cells of every leaf-ordered triangle (the bits follow the lights, lit_prepare)
        if ((rc = lit_resubdivide(r)) != PT_OK) return rc;
        // skip table: built with the scene where the mode uses it (pt_skip.h)
        if ((rc = skip_prepare(r)) != PT_OK) return rc;
    }
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return PT_OK;
}

int commit_geometry(pt_renderer* r, int how) {
    // the kernels already enqueued read the arrays about to be overwritten: stop a speculative
    // batch, then wait for every stream
    cancel_look_ahead(r, true);
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    for (int k = 1; k < pt_renderer::kMaxWFStreams; ++k)
        if (r->xstream[k]) PT_HIP(hipStreamSynchronize(r->xstream[k]), "hipStreamSynchronize");
    if (r->dl_stream) PT_HIP(hipStreamSynchronize(r->dl_stream), "hipStreamSynchronize");
    int rc = collect_pending(r);
    if (rc) return rc;

    std::vector<RefitMesh> rm((size_t)std::max(1, r->nmesh));
    if ((rc = apply_staged(r, rm)) != PT_OK) return rc;
    r->geom.any_staged = false;
    r->geom.version++;
    r->geom.commits++;
    r->geom.commit_ms = 0.0;
    if (r->ntri <= 0) {  // nothing to trace: the retained scene alone changed
        if (how == PT_GEOM_REBUILD) r->geom.rebuilds++;
        else r->geom.refits++;
        return PT_OK;
    }

    PT_HIP(hipMemcpy(r->d_mats, r->geom.mats.data(), sizeof(float4) * r->geom.mats.size(), hipMemcpyHostToDevice),
           "upload mats");
    if ((rc = need_tex_kernels(r)) != PT_OK) return rc;
    // refit: re-bake the dirty meshes' records, every node box bottom-up, the SAH cost
    PT_HIP(hipMemcpy(r->geom.d_rmesh, rm.data(), sizeof(RefitMesh) * rm.size(), hipMemcpyHostToDevice),
           "upload mesh records");
    PT_HIP(hipEventRecord(r->geom.ev[0], r->stream), "hipEventRecord");
    PT_HIP(refit_rebake(r->geom.d_rmesh, r->geom.d_overts, r->geom.d_onorms, r->geom.d_tidx, r->ntri, r->d_isect,
                        r->d_shade, r->stream),
           "k_rebake");
    PT_HIP(refit_levels(r->d_nodes, r->d_isect, r->geom.level_base, r->stream), "k_refit_level");
    if ((rc = sah_cost_now(r, false, r->geom.ev[1])) != PT_OK) return rc;
    float ms = 0.0f;
    PT_HIP(hipEventElapsedTime(&ms, r->geom.ev[0], r->geom.ev[1]), "hipEventElapsedTime");
    r->geom.commit_ms = ms;

    int rebuild_rc = PT_OK;
    std::string rebuild_msg;
    if (how == PT_GEOM_REBUILD) {
        rebuild_rc = rebuild_tree(r);
        if (rebuild_rc != PT_OK) rebuild_msg = g_last_error;
        if (rebuild_rc == PT_OK && (rc = sah_cost_now(r, true)) != PT_OK) return rc;
    }
    if (how == PT_GEOM_REBUILD && rebuild_rc == PT_OK) r->geom.rebuilds++;
    else r->geom.refits++;

    // the lit table's cells follow the records in force; its bits are rebuilt by the next call
    if ((rc = lit_resubdivide(r)) != PT_OK) return rc;
    // the skip table names links of the tree now in force: rebuilt here, outside any timed render call
    if ((rc = skip_prepare(r)) != PT_OK) return rc;
    if (rebuild_rc != PT_OK) return fail(rebuild_rc, rebuild_msg);
    return PT_OK;
}

}  // namespace pt
