// pt_capi.cpp — the C ABI of libptamd.so (include/ptamd.h): host driver for the gfx950
// path tracer.  Replaces Renderer/OptiX/OptixRenderer.{h,cpp} of Damo12320/OptixPathtracer
// (context/module/pipeline/SBT setup collapse into: upload scene -> BVH build -> launch).
//
// There is no CPU fallback: every render and trace call runs the HIP kernels or fails
// with a negative status.
#include "pt_renderer.h"

using namespace pt;

namespace pt {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
// Device allocations that fail for lack of memory report PT_ERR_NOMEM (the caller can retry
// with fewer frames per launch); every other HIP failure is PT_ERR_HIP.
int hip_fail(hipError_t e, const char* where) {
    g_last_error = std::string(where) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP;
}

}  // namespace pt

namespace {

// fp64 sum buffers (pt_set_accum_fp64) of one device for a W x H image, zeroed
int alloc_accum64(pt_renderer* r, int width, int height) {
    const size_t n = 3 * (size_t)width * (size_t)height;
    r->d_accum64.reset();  // both old buffers go before either new one is allocated
    r->multi.d_part64.reset();
    PT_HIP(r->d_accum64.alloc(n), "hipMalloc fp64 accum");
    PT_HIP(hipMemsetAsync(r->d_accum64, 0, sizeof(double) * n, r->stream), "hipMemset fp64 accum");
    if (!r->multi.comms.empty()) {
        PT_HIP(r->multi.d_part64.alloc(n), "hipMalloc fp64 partial sum");
        PT_HIP(hipMemsetAsync(r->multi.d_part64, 0, sizeof(double) * n, r->stream), "hipMemset fp64 partial sum");
    }
    return PT_OK;
}

bool valid_mode(int m) { return m >= PT_MAT_DEFAULT && m <= PT_MAT_LAYERED; }

// pt_create's options, before the device is opened.  devlist: the devices of a multi-device renderer.
int check_options(pt_options& opt, std::vector<int>& devlist) {
    // multi-device: validate the list, build device 0 here and the others as peers below
    if (opt.n_devices < 0) return fail(PT_ERR_INVALID, "pt_create: negative n_devices");
    for (int g = 0; g < opt.n_devices; ++g) devlist.push_back(opt.device_list ? opt.device_list[g] : opt.device + g);
    if (!devlist.empty()) opt.device = devlist[0];
    if (!valid_mode(opt.material_mode)) return fail(PT_ERR_INVALID, "pt_create: invalid material_mode");
    if (opt.bvh_builder != PT_BVH_AUTO && opt.bvh_builder != PT_BVH_PLOC && opt.bvh_builder != PT_BVH_LBVH &&
        opt.bvh_builder != PT_BVH_SAH && opt.bvh_builder != PT_BVH_SAH_GPU)
        return fail(PT_ERR_INVALID, "pt_create: invalid bvh_builder");
    if (opt.kernel != PT_KERNEL_MEGA && opt.kernel != PT_KERNEL_WAVEFRONT && opt.kernel != PT_KERNEL_AUTO)
        return fail(PT_ERR_INVALID, "pt_create: invalid kernel");
    return PT_OK;
}

// The devices exist and differ; opt.device becomes the current one.
int open_device(const pt_options& opt, const std::vector<int>& devlist) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(PT_ERR_HIP, "pt_create: no HIP device available");
    if (opt.device < 0 || opt.device >= ndev) return fail(PT_ERR_INVALID, "pt_create: device out of range");
    for (size_t g = 0; g < devlist.size(); ++g) {
        if (devlist[g] < 0 || devlist[g] >= ndev) return fail(PT_ERR_INVALID, "pt_create: device_list entry out of range");
        for (size_t h = 0; h < g; ++h)
            if (devlist[h] == devlist[g]) return fail(PT_ERR_INVALID, "pt_create: device_list repeats a device");
    }
    PT_HIP(hipSetDevice(opt.device), "hipSetDevice");
    return PT_OK;
}

// one single-device renderer per further device (own stream, scene copy, BVH build --
// the build is deterministic, so every device traces the same BVH), and one RCCL
// communicator over the list (ncclCommInitAll: a clique in this process)
int create_peers(pt_renderer* r, const pt_scene* scene, const pt_options& opt, std::vector<int>& devlist) {
    for (size_t g = 1; g < devlist.size(); ++g) {
        pt_options po = opt;
        po.device = devlist[g];
        po.n_devices = 0;
        po.device_list = nullptr;
        pt_renderer* p = nullptr;
        int rc = pt_create(scene, &po, &p);
        if (rc) return fail(rc, "pt_create (device " + std::to_string(devlist[g]) + "): " + std::string(g_last_error));
        r->multi.peers.push_back(p);
    }
    r->multi.comms.assign(devlist.size(), nullptr);
    const ncclResult_t nr = ncclCommInitAll(r->multi.comms.data(), (int)devlist.size(), devlist.data());
    if (nr != ncclSuccess) {
        r->multi.comms.clear();
        return fail(PT_ERR_HIP, std::string("pt_create: ncclCommInitAll: ") + ncclGetErrorString(nr));
    }
    (void)hipSetDevice(r->device);
    return PT_OK;
}

// pt_create's renderer until it is complete: a failure on the way destroys it.
struct CreateGuard {
    pt_renderer* r;
    ~CreateGuard() {
        if (r) pt_destroy(r);
    }
    pt_renderer* release() {
        pt_renderer* p = r;
        r = nullptr;
        return p;
    }
};

}  // namespace

namespace pt {

// glm::inverse (detail/func_matrix.inl compute_inverse<4,4>) in fp32, operation for operation: the
// inverses that pt_camera_from_blender hands out, and the ones pt_denoise_temporal takes of them.
void mat4_inverse(const float* m, float* out) {
    auto M = [&](int c, int r) { return m[c * 4 + r]; };
    float C00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3), C02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3);
    float C03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3), C04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3);
    float C06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3), C07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3);
    float C08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2), C10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2);
    float C11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2), C12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3);
    float C14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3), C15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3);
    float C16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2), C18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2);
    float C19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2), C20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1);
    float C22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1), C23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
    const float F0[4] = {C00, C00, C02, C03}, F1[4] = {C04, C04, C06, C07}, F2[4] = {C08, C08, C10, C11};
    const float F3[4] = {C12, C12, C14, C15}, F4[4] = {C16, C16, C18, C19}, F5[4] = {C20, C20, C22, C23};
    const float V0[4] = {M(1, 0), M(0, 0), M(0, 0), M(0, 0)}, V1[4] = {M(1, 1), M(0, 1), M(0, 1), M(0, 1)};
    const float V2[4] = {M(1, 2), M(0, 2), M(0, 2), M(0, 2)}, V3[4] = {M(1, 3), M(0, 3), M(0, 3), M(0, 3)};
    const float SA[4] = {+1, -1, +1, -1}, SB[4] = {-1, +1, -1, +1};
    float I0[4], I1[4], I2[4], I3[4];
    for (int i = 0; i < 4; ++i) {
        I0[i] = (V1[i] * F0[i] - V2[i] * F1[i] + V3[i] * F2[i]) * SA[i];
        I1[i] = (V0[i] * F0[i] - V2[i] * F3[i] + V3[i] * F4[i]) * SB[i];
        I2[i] = (V0[i] * F1[i] - V1[i] * F3[i] + V3[i] * F5[i]) * SA[i];
        I3[i] = (V0[i] * F2[i] - V1[i] * F4[i] + V2[i] * F5[i]) * SB[i];
    }
    float d0 = M(0, 0) * I0[0], d1 = M(0, 1) * I1[0], d2 = M(0, 2) * I2[0], d3 = M(0, 3) * I3[0];
    float one = 1.0f / ((d0 + d1) + (d2 + d3));
    for (int i = 0; i < 4; ++i) {
        out[i] = I0[i] * one;
        out[4 + i] = I1[i] * one;
        out[8 + i] = I2[i] * one;
        out[12 + i] = I3[i] * one;
    }
}

}  // namespace pt

extern "C" {

const char* pt_last_error(void) { return g_last_error.c_str(); }
const char* pt_version(void) { return "ptamd 0.1.0 gfx950"; }

int pt_create(const pt_scene* scene, const pt_options* options, pt_renderer** out) {
    if (!out) return fail(PT_ERR_INVALID, "pt_create: out is NULL");
    *out = nullptr;
    if (!scene || scene->n_meshes < 0 || (scene->n_meshes > 0 && !scene->meshes))
        return fail(PT_ERR_INVALID, "pt_create: invalid scene");
    pt_options opt{};
    if (options) opt = *options;
    std::vector<int> devlist;
    int rc = check_options(opt, devlist);
    if (rc == PT_OK) rc = open_device(opt, devlist);
    if (rc != PT_OK) return rc;

    std::vector<int4> texinfo;
    size_t ntexel = 0;
    bool any_tex = false;
    std::string err;
    GeomHost G;
    std::vector<float4> mats;
    if ((rc = ingest_scene(scene, G, mats, texinfo, &ntexel, &any_tex, &err)) != PT_OK) return fail(rc, err);

    CreateGuard g{new pt_renderer()};
    pt_renderer* r = g.r;
    r->geom.host = std::move(G);
    r->geom.mats = std::move(mats);
    // A/B switch for the wide trace workgroups (tools/ab.sh runs one library with and without)
    if (const char* e = std::getenv("PTAMD_WIDE_TRACE")) r->wide_trace = std::atoi(e) != 0;
    r->device = opt.device;
    r->material_mode = opt.material_mode;
    r->kernel = opt.kernel;
    r->ntri = (int)r->geom.host.tidx.size();
    r->nmesh = scene->n_meshes;
    r->geom.builder = opt.bvh_builder == PT_BVH_LBVH   ? kBuilderLBVH
                      : opt.bvh_builder == PT_BVH_PLOC ? kBuilderPLOC
                      : opt.bvh_builder == PT_BVH_SAH  ? kBuilderSAH
                                                       : kBuilderSAHGPU;
    r->geom.staged.resize((size_t)std::max(0, scene->n_meshes));
    if ((rc = upload_scene(r, scene, texinfo, ntexel)) != PT_OK) return rc;
    if ((rc = build_scene(r, any_tex)) != PT_OK) return rc;
    if (!devlist.empty() && (rc = create_peers(r, scene, opt, devlist)) != PT_OK) return rc;
    *out = g.release();
    return PT_OK;
}

// What is about order; every resource releases itself when the renderer is deleted.
int pt_destroy(pt_renderer* r) {
    if (!r) return PT_OK;
    if (r->ahead.hold.h) __atomic_store_n(r->ahead.hold.h, 1u, __ATOMIC_SEQ_CST);  // a held batch ends now
    for (pt_renderer* p : r->multi.peers) (void)hipSetDevice(p->device), (void)hipStreamSynchronize(p->stream);
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    for (ncclComm_t c : r->multi.comms)
        if (c) (void)ncclCommDestroy(c);
    for (pt_renderer* p : r->multi.peers) pt_destroy(p);
    (void)hipSetDevice(r->device);
    delete r;
    return PT_OK;
}

int pt_resize(pt_renderer* r, int32_t width, int32_t height) {
    if (!r) return fail(PT_ERR_INVALID, "pt_resize: NULL renderer");
    if (width < 0 || height < 0) return fail(PT_ERR_INVALID, "pt_resize: negative size");
    if (width == 0 || height == 0) return PT_OK;  // minimised window: no-op (OptixRenderer.cpp:651)
    if (filter_image_too_large(r->filter.set.supersample, width, height))
        return fail(PT_ERR_INVALID, "pt_resize: with the pixel filter set, supersample^2 * width * height must stay below 2^31");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_resize(p, width, height);
        if (rc) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    cancel_look_ahead(r, true);  // the wait below must not sit behind speculative frames
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    const size_t n3 = 3 * (size_t)width * (size_t)height, bytes = sizeof(float) * n3;
    // everything of the old size goes before anything of the new size is allocated
    r->d_frame.reset();
    ring_free(r);
    r->d_accum.reset();
    r->d_display.reset();
    r->aov.release();
    r->temporal.release();
    r->adaptive.release();
    r->multi.d_part.reset();
    r->d_accum64.reset();
    r->multi.d_part64.reset();
    r->display_ready = false;
    // the size is committed only once every buffer exists (a failed allocation leaves an
    // unsized renderer, on which the render calls return PT_ERR_STATE)
    r->width = r->height = 0;
    r->user_accum = nullptr;
    r->nf_fit = 0;  // a new size: the queues may fit the full batch again
    PT_HIP(r->d_frame.alloc(n3), "hipMalloc frame");
    PT_HIP(r->d_accum.alloc(n3), "hipMalloc accum");
    PT_HIP(hipMemsetAsync(r->d_accum, 0, bytes, r->stream), "hipMemset accum");
    if (!r->multi.comms.empty()) {
        PT_HIP(r->multi.d_part.alloc(n3), "hipMalloc partial sum");
        PT_HIP(hipMemsetAsync(r->multi.d_part, 0, bytes, r->stream), "hipMemset partial sum");
    }
    if (r->accum64) {
        const int rc = alloc_accum64(r, width, height);
        if (rc) return rc;
    }
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    r->width = width;
    r->height = height;
    return PT_OK;
}

int pt_set_camera(pt_renderer* r, const float position[3], const float inverse_view[16],
                  const float inverse_projection[16]) {
    if (!r || !position || !inverse_view || !inverse_projection) return fail(PT_ERR_INVALID, "pt_set_camera: NULL");
    std::memcpy(r->cam_pos, position, sizeof r->cam_pos);
    std::memcpy(r->inv_view, inverse_view, sizeof r->inv_view);
    std::memcpy(r->inv_proj, inverse_projection, sizeof r->inv_proj);
    for (pt_renderer* p : r->multi.peers) (void)pt_set_camera(p, position, inverse_view, inverse_projection);
    cancel_look_ahead(r);  // a moved camera: the look-ahead frames in flight are stale
    return PT_OK;
}

int pt_set_lights(pt_renderer* r, const pt_point_light* lights, int32_t count) {
    if (!r || count < 0 || (count > 0 && !lights)) return fail(PT_ERR_INVALID, "pt_set_lights: invalid");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_set_lights(p, lights, count);
        if (rc) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    cancel_look_ahead(r, true);  // new lights: the upload below must not wait behind speculative frames
    if ((size_t)count > r->lights_own.size()) {
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
        // no lights until the new array exists (a failed allocation must not leave a stale
        // count over a NULL array)
        r->d_lights = nullptr;
        r->n_lights = 0;
        PT_HIP(r->lights_own.alloc((size_t)count), "hipMalloc lights");
        r->d_lights = r->lights_own;
    }
    if (count > 0) {
        std::vector<DevLight> h((size_t)count);
        for (int i = 0; i < count; ++i)
            h[i] = DevLight{lights[i].position[0], lights[i].position[1], lights[i].position[2],
                            lights[i].color[0],    lights[i].color[1],    lights[i].color[2]};
        PT_HIP(hipMemcpyAsync(r->d_lights, h.data(), sizeof(DevLight) * (size_t)count, hipMemcpyHostToDevice,
                              r->stream),
               "upload lights");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    }
    r->n_lights = count;
    r->lights_version++;  // new contents, possibly in the same array: the render-ahead ring is stale
    r->lit.version++;     // and so are the lit table's bits: rebuilt here, outside any timed render call
    return lit_prepare(r);
}

int pt_set_max_bounces(pt_renderer* r, int32_t max_bounces) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_max_bounces: NULL");
    // SetMaxBounces (OptixRenderer.cpp:677-679) takes any int; a negative count would never
    // enter SamplePath's loop, like 0, so it is rejected here rather than silently renamed
    if (max_bounces < 0) return fail(PT_ERR_INVALID, "pt_set_max_bounces: negative count");
    r->max_bounces = max_bounces;
    for (pt_renderer* p : r->multi.peers) p->max_bounces = max_bounces;
    cancel_look_ahead(r);
    return PT_OK;
}

int pt_set_material_mode(pt_renderer* r, int32_t mode) {
    if (!r || !valid_mode(mode)) return fail(PT_ERR_INVALID, "pt_set_material_mode: invalid");
    r->material_mode = mode;
    for (pt_renderer* p : r->multi.peers) p->material_mode = mode;
    cancel_look_ahead(r);
    return PT_OK;
}

int pt_set_kernel(pt_renderer* r, int32_t kernel) {
    if (!r || (kernel != PT_KERNEL_MEGA && kernel != PT_KERNEL_WAVEFRONT && kernel != PT_KERNEL_AUTO))
        return fail(PT_ERR_INVALID, "pt_set_kernel: invalid");
    r->kernel = kernel;
    for (pt_renderer* p : r->multi.peers) p->kernel = kernel;
    cancel_look_ahead(r);
    return PT_OK;
}

int pt_set_mesh_transform(pt_renderer* r, int32_t mesh, const float model_matrix[16]) {
    if (!r || !model_matrix) return fail(PT_ERR_INVALID, "pt_set_mesh_transform: NULL");
    if (mesh < 0 || mesh >= r->nmesh) return fail(PT_ERR_INVALID, "pt_set_mesh_transform: mesh out of range");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_set_mesh_transform(p, mesh, model_matrix);
        if (rc) return rc;
    }
    StagedMesh& sm = r->geom.staged[(size_t)mesh];
    std::memcpy(sm.model, model_matrix, sizeof sm.model);
    sm.has_model = true;
    r->geom.any_staged = true;
    return PT_OK;
}

int pt_set_mesh_vertices(pt_renderer* r, int32_t mesh, const float* vertices, const float* normals) {
    if (!r || !vertices) return fail(PT_ERR_INVALID, "pt_set_mesh_vertices: NULL");
    if (mesh < 0 || mesh >= r->nmesh) return fail(PT_ERR_INVALID, "pt_set_mesh_vertices: mesh out of range");
    if (normals && !r->geom.host.has_normals[(size_t)mesh])
        return fail(PT_ERR_INVALID, "pt_set_mesh_vertices: the mesh was created without normals");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_set_mesh_vertices(p, mesh, vertices, normals);
        if (rc) return rc;
    }
    const size_t nv = (size_t)(r->geom.host.voff[(size_t)mesh + 1] - r->geom.host.voff[(size_t)mesh]);
    StagedMesh& sm = r->geom.staged[(size_t)mesh];
    sm.verts.assign(vertices, vertices + 3 * nv);
    sm.has_verts = true;
    if (normals) {
        sm.norms.assign(normals, normals + 3 * nv);
        sm.has_norms = true;
    }
    r->geom.any_staged = true;
    return PT_OK;
}

int pt_commit_geometry(pt_renderer* r, int32_t how) {
    if (!r) return fail(PT_ERR_INVALID, "pt_commit_geometry: NULL renderer");
    if (how != PT_GEOM_REFIT && how != PT_GEOM_REBUILD)
        return fail(PT_ERR_INVALID, "pt_commit_geometry: how must be PT_GEOM_REFIT or PT_GEOM_REBUILD");
    if (!r->geom.any_staged) return PT_OK;
    // every peer applies the same staged changes (the setters forwarded them) on its own device
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_commit_geometry(p, how);
        if (rc) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    return commit_geometry(r, how);
}


int pt_render(pt_renderer* r, float* host_rgb) {
    if (!r) return fail(PT_ERR_INVALID, "pt_render: NULL renderer");
    if (r->width == 0) return PT_OK;  // OptixRenderer.cpp:621
    if (!host_rgb) return fail(PT_ERR_INVALID, "pt_render: NULL output");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    r->frame_id++;  // :623
    size_t bytes = sizeof(float) * 3 * (size_t)r->width * (size_t)r->height;
    const float* img = nullptr;
    hipEvent_t ready = nullptr, part = nullptr;
    size_t part_floats = 0;
    int rc = render_frame_image(r, &img, &ready, true, &part, &part_floats);
    if (rc) return rc;
    // the download runs on its own stream after the image's event, so a look-ahead batch that
    // render_frame_image enqueued on r->stream keeps rendering while this frame is copied
    if (!r->dl_stream) PT_HIP(r->dl_stream.create(), "hipStreamCreate");
    if (part) {  // a banded frame: its first band's rows while the second band renders
        PT_HIP(hipStreamWaitEvent(r->dl_stream, part, 0), "hipStreamWaitEvent");
        PT_HIP(hipMemcpyAsync(host_rgb, img, sizeof(float) * part_floats, hipMemcpyDeviceToHost, r->dl_stream),
               "download frame");
        host_rgb += part_floats;
        img += part_floats;
        bytes -= sizeof(float) * part_floats;
    }
    PT_HIP(hipStreamWaitEvent(r->dl_stream, ready, 0), "hipStreamWaitEvent");
    PT_HIP(hipMemcpyAsync(host_rgb, img, bytes, hipMemcpyDeviceToHost, r->dl_stream), "download frame");
    PT_HIP(hipStreamSynchronize(r->dl_stream), "hipStreamSynchronize");
    // with a look-ahead batch in flight the launch events are retired later (pt_get_stats, a
    // synchronising call, or launch_frames' kMaxPendingEvents bound), not by waiting for it here
    return r->ahead.spec_pending ? PT_OK : collect_pending(r);
}

int pt_launch(pt_renderer* r, const pt_launch_params* lp) {
    static_assert(sizeof(pt_point_light) == sizeof(DevLight), "pt_point_light is read as DevLight on the device");
    if (!r || !lp) return fail(PT_ERR_INVALID, "pt_launch: NULL");
    const int w = lp->frame.size[0], h = lp->frame.size[1];
    if (w < 0 || h < 0 || lp->point_light_count < 0 || lp->max_bounces < 0)
        return fail(PT_ERR_INVALID, "pt_launch: negative size, light count or max bounces");
    if (w == 0 || h == 0) return PT_OK;  // an empty launch grid
    if (!lp->frame.color_buffer || (lp->point_light_count > 0 && !lp->point_lights))
        return fail(PT_ERR_INVALID, "pt_launch: NULL color buffer or lights");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    // this launch's state replaces the renderer's for the duration of the enqueue only
    const int ow = r->width, oh = r->height, on = r->n_lights, ob = r->max_bounces;
    float opos[3], oview[16], oproj[16];
    std::memcpy(opos, r->cam_pos, sizeof opos);
    std::memcpy(oview, r->inv_view, sizeof oview);
    std::memcpy(oproj, r->inv_proj, sizeof oproj);
    DevLight* olights = r->d_lights;
    r->width = w;
    r->height = h;
    std::memcpy(r->cam_pos, lp->camera.position, sizeof r->cam_pos);
    std::memcpy(r->inv_view, lp->camera.inverse_view_matrix, sizeof r->inv_view);
    std::memcpy(r->inv_proj, lp->camera.inverse_projection_matrix, sizeof r->inv_proj);
    r->d_lights = reinterpret_cast<DevLight*>(const_cast<pt_point_light*>(lp->point_lights));
    r->n_lights = lp->point_light_count;
    r->max_bounces = lp->max_bounces;
    r->lit.launch_call = true;
    if (r->lit.mode > 0) r->lit.version++;  // forced on: the array's contents may differ from call to call
    // colorBuffer[fbIndex] = pathRadiance (devicePrograms.cu:705): a one-frame sum into zeros
    hipError_t e = hipMemsetAsync(lp->frame.color_buffer, 0, sizeof(float) * 3 * (size_t)w * (size_t)h, r->stream);
    FrameCall c;
    c.first = lp->frame.id;
    c.n = 1;
    c.accum = lp->frame.color_buffer;
    int rc = e == hipSuccess ? launch_frames(r, c)
                             : fail(PT_ERR_HIP, std::string("pt_launch: hipMemsetAsync: ") + hipGetErrorString(e));
    r->width = ow;
    r->height = oh;
    std::memcpy(r->cam_pos, opos, sizeof opos);
    std::memcpy(r->inv_view, oview, sizeof oview);
    std::memcpy(r->inv_proj, oproj, sizeof oproj);
    r->d_lights = olights;
    r->n_lights = on;
    r->max_bounces = ob;
    r->lit.launch_call = false;
    return rc;
}

int pt_display_reset(pt_renderer* r, int32_t max_samples) {
    if (!r) return fail(PT_ERR_INVALID, "pt_display_reset: NULL");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_display_reset: call pt_resize first");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    const size_t n = 3 * (size_t)r->width * (size_t)r->height;
    if (!r->d_display) PT_HIP(r->d_display.alloc(n), "hipMalloc display");
    PT_HIP(display_fill(r->d_display, n, 1.0f, r->stream), "display clear");  // glClearColor(1,1,1,1)
    r->display_max = max_samples;
    r->display_samples = 0;
    r->display_ready = true;
    return PT_OK;
}

int pt_display_add_frame(pt_renderer* r, int32_t* samples) {
    if (!r) return fail(PT_ERR_INVALID, "pt_display_add_frame: NULL");
    if (!r->display_ready) return fail(PT_ERR_STATE, "pt_display_add_frame: call pt_display_reset first");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    r->frame_id++;  // Render: OptixRenderer.cpp:623
    const size_t n = 3 * (size_t)r->width * (size_t)r->height;
    const float* img = nullptr;
    int rc = render_frame_image(r, &img);
    if (rc) return rc;
    r->display_samples++;  // OptixView.cpp:239-248
    const bool continuous = r->display_max < 0;
    const float w = continuous ? 1.0f / (float)r->display_samples : 1.0f / (float)r->display_max;
    PT_HIP(display_blend(r->d_display, img, n, w, continuous, r->stream), "display blend");
    if (samples) *samples = r->display_samples;
    return PT_OK;
}

int pt_display_download(pt_renderer* r, float* host_rgb) {
    if (!r || !host_rgb) return fail(PT_ERR_INVALID, "pt_display_download: NULL");
    if (!r->display_ready) return fail(PT_ERR_STATE, "pt_display_download: call pt_display_reset first");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    const size_t bytes = sizeof(float) * 3 * (size_t)r->width * (size_t)r->height;
    PT_HIP(hipMemcpyAsync(host_rgb, r->d_display, bytes, hipMemcpyDeviceToHost, r->stream), "download display");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return collect_pending(r);
}

int pt_accum_clear(pt_renderer* r) {
    if (!r) return fail(PT_ERR_INVALID, "pt_accum_clear: NULL");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_accum_clear: call pt_resize first");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_accum_clear(p);
        if (rc) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    size_t bytes = sizeof(float) * 3 * (size_t)r->width * (size_t)r->height;
    r->adaptive.valid = false;  // the counts and moments described the sum that goes
    PT_HIP(hipMemsetAsync(r->accum(), 0, bytes, r->stream), "hipMemset accum");
    if (r->multi.d_part) PT_HIP(hipMemsetAsync(r->multi.d_part, 0, bytes, r->stream), "hipMemset partial sum");
    if (r->d_accum64) PT_HIP(hipMemsetAsync(r->d_accum64, 0, 2 * bytes, r->stream), "hipMemset fp64 accum");
    if (r->multi.d_part64) PT_HIP(hipMemsetAsync(r->multi.d_part64, 0, 2 * bytes, r->stream), "hipMemset fp64 partial sum");
    return PT_OK;
}

int pt_render_frames(pt_renderer* r, uint32_t first_frame_id, uint32_t n_frames) {
    if (!r) return fail(PT_ERR_INVALID, "pt_render_frames: NULL");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_render_frames: call pt_resize first");
    if (n_frames == 0) return PT_OK;
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    if (!r->multi.comms.empty()) return render_frames_multi(r, first_frame_id, n_frames);
    FrameCall c;
    c.first = first_frame_id;
    c.n = n_frames;
    c.accum = r->accum();
    if (r->accum64) c.accum64 = r->d_accum64;
    return launch_frames(r, c);
}

int pt_render_accumulate(pt_renderer* r, uint32_t spp, uint32_t first_frame_id, float* host_rgb_mean) {
    if (!r) return fail(PT_ERR_INVALID, "pt_render_accumulate: NULL");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_render_accumulate: call pt_resize first");
    if (spp == 0) return fail(PT_ERR_INVALID, "pt_render_accumulate: spp must be > 0");
    int rc = pt_accum_clear(r);
    if (rc) return rc;
    rc = pt_render_frames(r, first_frame_id, spp);
    if (rc) return rc;
    if (host_rgb_mean) return pt_accum_download(r, host_rgb_mean, 1.0f / (float)spp);
    return pt_synchronize(r);
}

int pt_set_accum_device_buffer(pt_renderer* r, float* device_sum_rgb) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_accum_device_buffer: NULL");
    r->user_accum = device_sum_rgb;
    return PT_OK;
}

float* pt_accum_device_ptr(pt_renderer* r) { return r ? r->accum() : nullptr; }

int pt_set_accum_fp64(pt_renderer* r, int32_t on) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_accum_fp64: NULL");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_set_accum_fp64(p, on);
        if (rc) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    r->accum64 = on != 0;
    if (r->accum64 && r->width > 0) {
        // start from the current fp32 sum (device 0 of a multi-device renderer: its own partial
        // sum, which the next reduce adds to the others'), so a switch keeps what is there
        const int rc = alloc_accum64(r, r->width, r->height);
        if (rc) return rc;
        const size_t n = 3 * (size_t)r->width * (size_t)r->height;
        std::vector<float> h32(n);
        std::vector<double> h64(n);
        const float* src = r->multi.comms.empty() ? r->accum() : r->multi.d_part;
        double* dst = r->multi.comms.empty() ? r->d_accum64 : r->multi.d_part64;
        // on the library stream, after alloc_accum64's zeroing: a null-stream hipMemcpy would not
        // wait for the non-blocking stream, and the memset could land on the seeded sum
        PT_HIP(hipMemcpyAsync(h32.data(), src, n * sizeof(float), hipMemcpyDeviceToHost, r->stream), "download accum");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
        for (size_t i = 0; i < n; ++i) h64[i] = (double)h32[i];
        PT_HIP(hipMemcpyAsync(dst, h64.data(), n * sizeof(double), hipMemcpyHostToDevice, r->stream),
               "upload fp64 accum");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    } else if (!r->accum64) {
        r->d_accum64.reset();
        r->multi.d_part64.reset();
    }
    return PT_OK;
}

double* pt_accum_device_ptr64(pt_renderer* r) { return r ? r->d_accum64 : nullptr; }

int pt_accum_download64(pt_renderer* r, double* host_rgb) {
    if (!r || !host_rgb) return fail(PT_ERR_INVALID, "pt_accum_download64: NULL");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_accum_download64: call pt_resize first");
    if (!r->d_accum64) return fail(PT_ERR_STATE, "pt_accum_download64: fp64 accumulation is off (pt_set_accum_fp64)");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    size_t n = 3 * (size_t)r->width * (size_t)r->height;
    PT_HIP(hipMemcpyAsync(host_rgb, r->d_accum64, n * sizeof(double), hipMemcpyDeviceToHost, r->stream),
           "download fp64 accum");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return collect_pending(r);
}

int pt_accum_download(pt_renderer* r, float* host_rgb, float scale) {
    if (!r || !host_rgb) return fail(PT_ERR_INVALID, "pt_accum_download: NULL");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_accum_download: call pt_resize first");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    size_t n = 3 * (size_t)r->width * (size_t)r->height;
    PT_HIP(hipMemcpyAsync(host_rgb, r->accum(), n * sizeof(float), hipMemcpyDeviceToHost, r->stream), "download accum");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    if (scale != 1.0f)
        for (size_t i = 0; i < n; ++i) host_rgb[i] *= scale;
    return collect_pending(r);
}

int pt_synchronize(pt_renderer* r) {
    if (!r) return fail(PT_ERR_INVALID, "pt_synchronize: NULL");
    for (pt_renderer* p : r->multi.peers) {
        const int rc = pt_synchronize(p);
        if (rc) return rc;
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return collect_pending(r);
}

void* pt_stream(pt_renderer* r) { return r ? (void*)r->stream : nullptr; }
int32_t pt_device_count(const pt_renderer* r) { return r ? (int32_t)(1 + r->multi.peers.size()) : 0; }
int pt_devices(const pt_renderer* r, int32_t* devices, int32_t max) {
    if (!r || max < 0 || (max > 0 && !devices)) return fail(PT_ERR_INVALID, "pt_devices: invalid");
    for (int32_t g = 0; g < max && g < pt_device_count(r); ++g) devices[g] = g == 0 ? r->device : r->multi.peers[g - 1]->device;
    return PT_OK;
}
uint32_t pt_frame_id(const pt_renderer* r) { return r ? r->frame_id : 0u; }
int pt_set_frame_id(pt_renderer* r, uint32_t frame_id) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_frame_id: NULL");
    r->frame_id = frame_id;
    return PT_OK;
}


int pt_set_render_ahead(pt_renderer* r, int32_t frames) {
    if (!r || frames < 1 || frames > 1024) return fail(PT_ERR_INVALID, "pt_set_render_ahead: frames must be 1..1024");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    ring_free(r);
    r->ahead.max_frames = frames;
    return PT_OK;
}

int pt_set_render_ahead_budget(pt_renderer* r, float max_ms) {
    if (!r || !(max_ms >= 0.0f)) return fail(PT_ERR_INVALID, "pt_set_render_ahead_budget: max_ms must be >= 0");
    r->ahead.budget_ms = max_ms;
    return PT_OK;
}

int pt_set_frames_per_launch(pt_renderer* r, int32_t frames) {
    if (!r || frames < 1) return fail(PT_ERR_INVALID, "pt_set_frames_per_launch: invalid");
    r->frames_per_launch = frames;
    r->nf_fit = 0;
    for (pt_renderer* p : r->multi.peers) {
        p->frames_per_launch = frames;
        p->nf_fit = 0;
    }
    return PT_OK;
}

int pt_get_trace_coherence(pt_renderer* r, uint64_t hist[8]) {
    if (!r || !hist) return fail(PT_ERR_INVALID, "pt_get_trace_coherence: NULL");
    int rc = pt_synchronize(r);
    if (rc) return rc;
    unsigned long long c[kCounters];
    PT_HIP(hipMemcpy(c, r->d_counters, sizeof c, hipMemcpyDeviceToHost), "download counters");
    uint64_t steps = 0;
    for (int k = 0; k < 6; ++k) {
        hist[k] = c[kCtrCoh0 + k];
        steps += c[kCtrCoh0 + k];
    }
    hist[6] = steps;
    hist[7] = c[kCtrCohLanes];
    for (pt_renderer* p : r->multi.peers) {  // a multi-device renderer: every device's steps
        uint64_t ph[8];
        if ((rc = pt_get_trace_coherence(p, ph)) != PT_OK) return rc;
        for (int k = 0; k < 8; ++k) hist[k] += ph[k];
    }
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    return PT_OK;
}

int pt_set_queue_budget(pt_renderer* r, int64_t bytes) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_queue_budget: NULL");
    r->queue_budget = bytes;
    for (pt_renderer* p : r->multi.peers) p->queue_budget = bytes;
    return PT_OK;
}

int pt_set_debug_hold(pt_renderer* r, int32_t on) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_debug_hold: NULL");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    if (!r->ahead.hold.h) {
        PT_HIP(r->ahead.hold.alloc(1u), "hipHostMalloc hold word");
        PT_HIP(r->ahead.hold.map(), "hipHostGetDevicePointer hold word");
    }
    // on: later speculative batches wait in k_hold; off: a batch waiting there goes on now
    __atomic_store_n(r->ahead.hold.h, on ? 0u : 1u, __ATOMIC_SEQ_CST);
    r->ahead.debug_hold = on != 0;
    return PT_OK;
}

int pt_camera_from_blender(const float bp[3], const float br[3], float fov_deg, int32_t W, int32_t H, float pos[3],
                           float inv_view[16], float inv_proj[16]) {
    if (!bp || !br || !pos || !inv_view || !inv_proj || W <= 0 || H <= 0)
        return fail(PT_ERR_INVALID, "pt_camera_from_blender: invalid");
    const float deg2rad = 0.01745329251994329576923690768489f;  // glm::radians
    f3 p = mk(bp[0], bp[2], -bp[1]);                             // GlmHelperMethods.cpp:4-6
    f3 rot = mk(90.0f - br[0], 180.0f + br[2], br[1]);           // GlmHelperMethods.cpp:8-10
    f3 rr = mk(rot.x * deg2rad, rot.y * deg2rad, rot.z * deg2rad);
    float x = sinf(rr.y);  // Camera::GetForward, Camera.cpp:37-49
    x *= cosf(rr.x);
    float y = -sinf(rr.x);
    float z = cosf(rr.x);
    z *= cosf(rr.y);
    f3 fwd = normalize(mk(x, y, z));
    // glm::lookAtRH(pos, pos + fwd, (0,1,0)) — Camera.cpp:64-66
    f3 center = p + fwd;
    f3 f = normalize(center - p);
    f3 s = normalize(cross(f, mk(0.0f, 1.0f, 0.0f)));
    f3 u = cross(s, f);
    float V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    V[0] = s.x; V[4] = s.y; V[8] = s.z;
    V[1] = u.x; V[5] = u.y; V[9] = u.z;
    V[2] = -f.x; V[6] = -f.y; V[10] = -f.z;
    V[12] = -dot(s, p); V[13] = -dot(u, p); V[14] = dot(f, p);
    // glm::perspectiveRH_NO(fovy, aspect, 0.1, 100) — Camera.cpp:68-70, OptixRenderer.cpp:663
    float fovy = fov_deg * deg2rad;
    float aspect = (float)W / (float)H;
    const float zn = 0.1f, zf = 100.0f;
    float th = tanf(fovy / 2.0f);
    float P[16] = {0};
    P[0] = 1.0f / (aspect * th);
    P[5] = 1.0f / th;
    P[10] = -(zf + zn) / (zf - zn);
    P[11] = -1.0f;
    P[14] = -(2.0f * zf * zn) / (zf - zn);
    pos[0] = p.x;
    pos[1] = p.y;
    pos[2] = p.z;
    mat4_inverse(V, inv_view);
    mat4_inverse(P, inv_proj);
    return PT_OK;
}

int pt_trace_rays(pt_renderer* r, const float* host_rays, int32_t n, int32_t* prim, float* t, float* u, float* v,
                  int32_t* backface, int32_t any_hit) {
    if (!r || n < 0 || (n > 0 && (!host_rays || !prim || !t || !u || !v || !backface)))
        return fail(PT_ERR_INVALID, "pt_trace_rays: invalid");
    if (n == 0) return PT_OK;
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    DevBuf<float> d_rays, d_t, d_u, d_v;
    DevBuf<int> d_p, d_b;
    size_t nn = (size_t)n;
    hipError_t e = d_rays.alloc(8 * nn);
    if (e == hipSuccess) e = d_t.alloc(nn);
    if (e == hipSuccess) e = d_u.alloc(nn);
    if (e == hipSuccess) e = d_v.alloc(nn);
    if (e == hipSuccess) e = d_p.alloc(nn);
    if (e == hipSuccess) e = d_b.alloc(nn);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays, host_rays, 8 * nn * sizeof(float), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = launch_trace(r->scene(), d_rays, n, d_p, d_t, d_u, d_v, d_b, any_hit, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(prim, d_p, nn * sizeof(int), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t, d_t, nn * sizeof(float), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(u, d_u, nn * sizeof(float), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v, d_v, nn * sizeof(float), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(backface, d_b, nn * sizeof(int), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return hip_fail(e, "pt_trace_rays");
    return PT_OK;
}

}  // extern "C"

extern "C" int pt_bvh_download(pt_renderer* r, void* nodes, int64_t node_bytes, void* triangles,
                               int64_t triangle_bytes) {
    if (!r || node_bytes < 0 || triangle_bytes < 0 || (node_bytes > 0 && !nodes) ||
        (triangle_bytes > 0 && !triangles))
        return fail(PT_ERR_INVALID, "pt_bvh_download: invalid");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    const int64_t nb = std::min<int64_t>(node_bytes, (int64_t)sizeof(BNode4) * r->bvh_nodes);
    const int64_t tb = std::min<int64_t>(triangle_bytes, (int64_t)sizeof(float4) * 3 * r->ntri);
    if (nb > 0) PT_HIP(hipMemcpy(nodes, r->d_nodes, (size_t)nb, hipMemcpyDeviceToHost), "download nodes");
    if (tb > 0) PT_HIP(hipMemcpy(triangles, r->d_isect, (size_t)tb, hipMemcpyDeviceToHost), "download triangles");
    return PT_OK;
}

extern "C" int pt_set_debug_pixel(pt_renderer* r, int32_t x, int32_t y, uint32_t frame_id) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_debug_pixel: NULL");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    if (x < 0 || y < 0) {  // off
        r->debug_pixel = -1;
        return PT_OK;
    }
    if (r->width == 0 || x >= r->width || y >= r->height)
        return fail(PT_ERR_INVALID, "pt_set_debug_pixel: pixel outside the frame (call pt_resize first)");
    const size_t bytes = sizeof(float) * kDebugRecordFloats * kDebugMaxBounces;
    if (!r->d_debug) PT_HIP(r->d_debug.alloc((size_t)kDebugRecordFloats * kDebugMaxBounces), "hipMalloc debug records");
    PT_HIP(hipMemset(r->d_debug, 0, bytes), "hipMemset debug records");
    r->debug_pixel = r->width * y + x;
    r->debug_frame = frame_id;
    r->debug_version++;  // records cleared: no ring image rendered before stands for this state
    return PT_OK;
}

extern "C" int pt_get_debug_path(pt_renderer* r, pt_debug_bounce* out, int32_t max, int32_t* n_bounces) {
    static_assert(sizeof(pt_debug_bounce) == sizeof(float) * kDebugRecordFloats, "pt_debug_bounce layout");
    if (!r || max < 0 || (max > 0 && !out) || !n_bounces) return fail(PT_ERR_INVALID, "pt_get_debug_path: invalid");
    *n_bounces = 0;
    if (!r->d_debug) return fail(PT_ERR_STATE, "pt_get_debug_path: call pt_set_debug_pixel first");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    std::vector<pt_debug_bounce> rec(kDebugMaxBounces);
    PT_HIP(hipMemcpy(rec.data(), r->d_debug, sizeof(pt_debug_bounce) * rec.size(), hipMemcpyDeviceToHost),
           "download debug records");
    int n = 0;
    while (n < kDebugMaxBounces && rec[(size_t)n].bounce == n + 1) ++n;
    *n_bounces = n;
    for (int k = 0; k < n && k < max; ++k) out[k] = rec[(size_t)k];
    return PT_OK;
}

extern "C" int pt_set_traversal_stats(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_traversal_stats: NULL");
    r->trav_stats = enable != 0;
    for (pt_renderer* p : r->multi.peers) p->trav_stats = enable != 0;
    return PT_OK;
}

extern "C" int pt_set_wavefront_streams(pt_renderer* r, int32_t streams) {
    if (!r || streams < 0 || streams > pt_renderer::kMaxWFStreams)
        return fail(PT_ERR_INVALID, "pt_set_wavefront_streams: 0 (auto) or 1 to 4");
    int rc = collect_pending(r);
    if (rc != PT_OK) return rc;
    r->wf_streams = streams;
    for (pt_renderer* p : r->multi.peers)
        if ((rc = pt_set_wavefront_streams(p, streams)) != PT_OK) return rc;
    return PT_OK;
}

extern "C" int pt_set_primary_dedup(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_primary_dedup: NULL");
    int rc = collect_pending(r);
    if (rc) return rc;
    r->primary_dedup = enable != 0;
    for (pt_renderer* p : r->multi.peers) {
        if ((rc = pt_set_primary_dedup(p, enable)) != PT_OK) return rc;
    }
    return PT_OK;
}

extern "C" int pt_set_lit_table(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_lit_table: NULL");
    const int mode = enable < 0 ? -1 : (enable > 0 ? 1 : 0);
    r->lit.mode = mode;  // the images do not depend on it: frames rendered ahead stay valid
    for (pt_renderer* p : r->multi.peers) p->lit.mode = mode;
    return PT_OK;
}

extern "C" int pt_lit_table_download(pt_renderer* r, pt_lit_table_info* info, uint32_t* tri_words, int64_t tri_bytes,
                                     uint32_t* bits, int64_t bits_bytes) {
    if (!r || !info) return fail(PT_ERR_INVALID, "pt_lit_table_download: NULL");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    return lit_table_download(r, info, tri_words, tri_bytes, bits, bits_bytes);
}

extern "C" int pt_set_occluder_table(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_occluder_table: NULL");
    const int mode = enable < 0 ? -1 : (enable > 0 ? 1 : 0);
    r->occ.mode = mode;  // the images do not depend on it: frames rendered ahead stay valid
    for (pt_renderer* p : r->multi.peers) p->occ.mode = mode;
    return PT_OK;
}

// The table for the renderer's state, built now if it is stale; *entries_out = lights * cells, 0 while
// it is not in use.  PT_ERR_INVALID for a buffer of another size.
extern "C" int pt_occluder_table_download(pt_renderer* r, int64_t* entries_out, int32_t* entries, int64_t bytes) {
    if (!r || !entries_out) return fail(PT_ERR_INVALID, "pt_occluder_table_download: NULL");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    return occ_table_download(r, entries_out, entries, bytes);
}

// Replaces the entries (lights * cells of them) until the next rebuild.  Every entry must be -1 or a
// leaf-order triangle index of the scene: anything else is rejected, nothing is written.
extern "C" int pt_occluder_table_upload(pt_renderer* r, const int32_t* entries, int64_t bytes) {
    if (!r || !entries) return fail(PT_ERR_INVALID, "pt_occluder_table_upload: NULL");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    int rc = occ_table_upload(r, entries, bytes);
    if (rc) return rc;
    for (pt_renderer* p : r->multi.peers) {
        if ((rc = pt_occluder_table_upload(p, entries, bytes)) != PT_OK) return rc;
    }
    return PT_OK;
}

extern "C" int pt_set_skip_table(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_skip_table: NULL");
    const int mode = enable < 0 ? -1 : (enable > 0 ? 1 : 0);
    r->skip.mode = mode;  // the images do not depend on it: frames rendered ahead stay valid
    for (pt_renderer* p : r->multi.peers) p->skip.mode = mode;
    return PT_OK;
}

// The words for the renderer's state, built now if they are stale; *words_out = 2 * triangles, 0 while
// the table is not in use.  PT_ERR_INVALID for a buffer of another size.
extern "C" int pt_skip_table_download(pt_renderer* r, int64_t* words_out, uint32_t* words, int64_t bytes) {
    if (!r || !words_out) return fail(PT_ERR_INVALID, "pt_skip_table_download: NULL");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    return skip_table_download(r, words_out, words, bytes);
}

extern "C" int pt_set_band_split(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_band_split: NULL");
    int rc = collect_pending(r);
    if (rc) return rc;
    r->band_split = enable != 0;
    for (pt_renderer* p : r->multi.peers) {
        if ((rc = pt_set_band_split(p, enable)) != PT_OK) return rc;
    }
    return PT_OK;
}

extern "C" int pt_set_kernel_timing(pt_renderer* r, int32_t enable) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_kernel_timing: NULL");
    int rc = collect_pending(r);
    if (rc) return rc;
    r->timing.kernel_timing = enable != 0;
    for (pt_renderer* p : r->multi.peers) {
        if ((rc = pt_set_kernel_timing(p, enable)) != PT_OK) return rc;
    }
    return PT_OK;
}
