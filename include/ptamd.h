/*
 * ptamd.h — C ABI of the MI355X-native path tracer (libptamd.so).
 *
 * Drop-in boundary for the render path of Damo12320/OptixPathtracer.  Each entry point
 * names the reference interface it replaces (paths relative to
 * OptixPathtracer/source/).  Plain C types only: pointers, sizes, int status codes.
 * Status: 0 = ok, < 0 = error (message via pt_last_error()).  Host pointers unless an
 * argument is documented as a device pointer.  Colour buffers are W*H*3 fp32, RGB
 * interleaved (glm::vec3 AoS as Renderer/OptiX/LaunchParams.h:12), row 0 = bottom
 * (OpenGL convention of devicePrograms.cu:607-608,704).
 */
#ifndef PTAMD_H
#define PTAMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_INVALID (-1)
#define PT_ERR_HIP (-2)
#define PT_ERR_STATE (-3)
#define PT_ERR_NOMEM (-4) /* a device allocation failed with hipErrorOutOfMemory (queues, frame or scene buffers) */

/* Material mode = which BSDF pair the closest-hit program uses.  The reference selects it
 * by (un)commenting lines in Renderer/OptiX/devicePrograms.cu:303-341. */
#define PT_MAT_DEFAULT 0    /* rnd < metallic ? Conductor : GlossyDiffuse (active reference code) */
#define PT_MAT_LAMBERT 1    /* devicePrograms.cu:306 / :326 */
#define PT_MAT_CONDUCTOR 2  /* devicePrograms.cu:307 / :327 */
#define PT_MAT_DIELECTRIC 3 /* devicePrograms.cu:304 / :324 */
#define PT_MAT_LAYERED 4    /* devicePrograms.cu:305 / :325 */

/* Render-kernel variants (all produce the same image). */
#define PT_KERNEL_MEGA 0      /* one thread per pixel, frames looped in registers */
#define PT_KERNEL_WAVEFRONT 1 /* wavefront: per-bounce kernels over SoA ray/hit queues, wave compaction */
#define PT_BVH_AUTO 0          /* default: PT_BVH_SAH_GPU */
#define PT_BVH_LBVH 1          /* GPU Karras LBVH -> BVH4 (fastest build) */
#define PT_BVH_SAH 2           /* host binned-SAH binary tree -> the GPU SAH-optimal BVH4 collapse: 13 %
                                  fewer node visits per ray than PLOC; 19 ms at 35k,
                                  115 ms at 250k triangles on one host thread.  The reference build of
                                  PT_BVH_SAH_GPU's tree. */
#define PT_BVH_PLOC 3          /* GPU PLOC clustering -> the same collapse (fast build, near-SAH)
                                  -- every builder gives the same images bit for bit */
#define PT_BVH_SAH_GPU 4       /* PT_BVH_SAH's tree built on the GPU (pt_sah_gpu.hip): the same BVH4 bit
                                  for bit.  Changelog: round 4 made 0 = AUTO (PLOC moved 0 -> 3);
                                  round 5 added this value and made it AUTO's choice. */

#define PT_KERNEL_AUTO 2      /* the faster path (measured): currently the wavefront in every mode */

/* Mesh: ModelLoading/Mesh.h:9-45 (vertecies, normal, texCoord, index, ModelMatrix, albedo,
 * metallic, roughness, texture ids).  Borrowed only during pt_create (deep copy). */
typedef struct pt_mesh {
    const float* vertices;    /* n_vertices * 3 */
    const float* normals;     /* n_vertices * 3, or NULL (reference then yields NaN shading normals) */
    const float* texcoords;   /* n_vertices * 2, or NULL */
    const int32_t* indices;   /* n_triangles * 3 (glm::ivec3 index, Mesh.h:20) */
    int32_t n_vertices;
    int32_t n_triangles;
    float model_matrix[16];   /* column-major glm::mat4 = Mesh::GetModelMatrix() (Mesh.cpp:6-22) */
    float albedo[3];
    float metallic;
    float roughness;
    int32_t albedo_tex;       /* -1 = none (Mesh.h:35-37) */
    int32_t normal_tex;
    int32_t metal_rough_tex;
} pt_mesh;

/* Texture: ModelLoading/Texture.h:5-12 (RGBA8 pixels). */
typedef struct pt_texture {
    const uint32_t* rgba8;
    int32_t width;
    int32_t height;
} pt_texture;

/* Model: ModelLoading/Model.h:5-8. */
typedef struct pt_scene {
    const pt_mesh* meshes;
    int32_t n_meshes;
    const pt_texture* textures;
    int32_t n_textures;
} pt_scene;

/* PointLight: Renderer/OptiX/LightsStruct.h:6-10. */
typedef struct pt_point_light {
    float position[3];
    float color[3];
} pt_point_light;

typedef struct pt_options {
    int32_t device;         /* HIP device ordinal (reference hard-codes device 0, OptixRenderer.cpp:70) */
    int32_t material_mode;  /* PT_MAT_* */
    int32_t kernel;         /* PT_KERNEL_* */
    int32_t bvh_builder;    /* PT_BVH_* (replaces optixAccelBuild, OptixRenderer.cpp:306-456) */
    /* Multi-GPU inside the library (SURVEY.md §8(b) threading row, §8(e)).  0: one device
     * (`device`), no RCCL.  n >= 1: the renderer drives n devices -- device_list[0..n), or
     * device .. device+n-1 when device_list is NULL -- each with its own HIP stream, scene copy
     * and BVH, plus one RCCL communicator over them created here.  pt_render_frames /
     * pt_render_accumulate split their frame ids into n contiguous blocks (device g renders
     * its block into its own fp32 sum) and ncclReduce the sums onto device_list[0], whose
     * buffer pt_accum_* read.  pt_render / pt_launch / pt_display_* run on device_list[0]. */
    int32_t n_devices;
    int32_t reserved[3];
    const int32_t* device_list;
} pt_options;

typedef struct pt_stats {
    uint64_t segments;        /* radiance rays traced (path segments) since pt_stats_reset */
    uint64_t samples;         /* camera paths since pt_stats_reset */
    double last_render_ms;    /* summed kernel time of the last render call */
    double total_render_ms;   /* summed kernel time since pt_stats_reset */
    uint64_t render_calls;    /* pt_render / pt_render_frames calls since pt_stats_reset */
    uint64_t kernel_launches; /* render-kernel launches since pt_stats_reset; each one is
                                 bracketed by its own HIP event pair on the library stream */
    double bvh_build_ms;      /* LBVH build + BVH4 collapse device time (pt_create) */
    int32_t bvh_nodes;        /* BVH4 inner nodes */
    int32_t triangles;
    int32_t frames_per_launch;
    int32_t bvh_depth;        /* BVH4 levels */
    /* traversal counters, only counted while pt_set_traversal_stats(r, 1) */
    uint64_t nodes_visited;
    uint64_t tri_tests;
    uint64_t rays;
    uint64_t stack_overflows;
    /* trace kernels of the wavefront path (k_extend, and k_trace_pair in the fused modes), only
       timed while pt_set_kernel_timing(r, 1): summed per-launch HIP-event time and launch count.
       A one-frame call in row bands (pt_set_band_split) times each band's launches separately,
       and the two bands run at the same time, so its per-launch times are per band and overlap
       (not comparable with a multi-frame call's). */
    double trace_kernel_ms;
    uint64_t trace_kernel_launches;
    uint64_t shadow_rays;        /* NEE shadow rays traced since pt_stats_reset */
    uint64_t trace_kernel_rays;  /* rays traced by the timed trace kernels (k_extend, k_trace_pair) */
    uint64_t trace_kernel_bytes; /* their algorithmic queue bytes: 32 B per ray read + 16 B per
                                    hit / shadow record written (k_extend with primary dedup
                                    writes one record per frame of the batch) */
    uint64_t strict_retraces;    /* always 0: no traversal traces a ray twice any more (every candidate
                                    hit is held to pt_device.h tri_accept_in as it is met); the field
                                    keeps the struct's layout */
    /* wave schedule of the lane-refilling trace kernels (k_extend, k_trace_pair),
       counted while pt_set_traversal_stats(r, 1): loop iterations of the waves, lanes with a ray
       in flight summed over them, iterations that ran the node half / the triangle half of the
       traversal step, and refill blocks.  nodes_visited / (64 * wave_node_steps) is the node
       half's lane utilisation. */
    uint64_t wave_steps;
    uint64_t wave_active_lanes;
    uint64_t wave_node_steps;
    uint64_t wave_tri_steps;
    uint64_t wave_refills;
    /* node visits of the wavefront trace kernels served from the top BVH levels staged in LDS
       (counted while pt_set_traversal_stats(r, 1)); nodes_visited - lds_nodes_visited loaded
       their 128-B node from global memory */
    uint64_t lds_nodes_visited;
    /* the bounce's dominant shading kernel of the wavefront path (k_shade_fused / k_shade0_pixel
       in the Lambert, Conductor and Dielectric modes; k_shade_nee, the layered NEE eval, in the
       Default and Layered modes), timed like the trace kernels while pt_set_kernel_timing(r, 1) */
    double shade_kernel_ms;
    uint64_t shade_kernel_launches;
    uint64_t shade_kernel_items; /* their queue items (hit records shaded; NEE items), always counted */
    /* render-ahead (pt_set_render_ahead): frames rendered into the ring, and pt_render /
       pt_display_add_frame calls served from it.  samples, segments and the kernel counters
       include every rendered frame, also those rendered ahead that no call has asked for yet
       (frames_rendered_ahead - frames_served_ahead of them at most). */
    uint64_t frames_rendered_ahead;
    uint64_t frames_served_ahead;
    /* look-ahead batches cancelled because the render state changed while they were in flight
       (their frames count in frames_rendered_ahead, but they stopped early) */
    uint64_t look_ahead_cancelled;
    /* the k_trace_pair launches alone (fused modes: every timed trace launch but the batch's
       k_extend), per kernel for the roofline: event time, launches, rays, algorithmic bytes
       (48 B per ray); included in trace_kernel_* as well */
    double pair_kernel_ms;
    uint64_t pair_kernel_launches;
    uint64_t pair_kernel_rays;
    uint64_t pair_kernel_bytes;
    /* the shadow rays among pair_kernel_rays (the rest are extension rays), and the shadow rays of
       k_trace_pair that found their light unoccluded (each adds its contribution to the path's
       radiance: a 16-B read and write; counted while pt_set_traversal_stats(r, 1)) */
    uint64_t pair_kernel_shadow_rays;
    uint64_t nee_unoccluded;
    /* round 6: device memory the wavefront queues of all streams hold now, and the queue budget
       in force (pt_set_queue_budget; 0 = none); the streams and frames per batch the last
       wavefront call actually used; speculative batches enqueued behind pt_set_debug_hold */
    uint64_t queue_bytes;
    uint64_t queue_budget;
    int32_t last_streams;
    int32_t last_batch_frames;
    uint64_t look_ahead_held;
    /* lit table (pt_set_lit_table): NEE visibility answers the shading kernels took from the table
       instead of tracing a shadow ray (shadow_rays, pair_kernel_shadow_rays and nee_unoccluded keep
       counting traced rays only); the table's cells per light, set bits over all lights, device
       bytes, and the device time of its last build (0 while no table is in use) */
    uint64_t lit_table_answers;
    uint64_t lit_table_cells;
    uint64_t lit_table_bits_set;
    uint64_t lit_table_bytes;
    double lit_table_build_ms;
    /* occluder candidate table (pt_set_occluder_table): device bytes, entries that name a triangle,
       device time of the last build (all 0 while the table is not in use), and the NEE tests a
       shading kernel answered "occluded" from it instead of emitting a shadow ray */
    uint64_t occluder_table_bytes;
    uint64_t occluder_table_candidates;
    double occluder_table_build_ms;
    uint64_t occluder_table_answers;
    /* skip table (pt_set_skip_table): device bytes of the words, device time of the last build (both 0
       while the table is not in use), and the extension rays that carried a skip link, counted by the
       traversal-statistics kernels like nodes_visited (0 in a render without them) */
    uint64_t skip_table_bytes;
    double skip_table_build_ms;
    uint64_t skip_table_rays;
    /* geometry updates (pt_commit_geometry): commits that changed something, how many of them ended on
       a refitted and how many on a rebuilt tree, and the device time of the last commit's work (HIP
       events around the re-bake, the level refits and the cost reduction, plus the build's own
       device time for a rebuild) */
    uint64_t geometry_commits;
    uint64_t geometry_refits;
    uint64_t geometry_rebuilds;
    double geometry_commit_ms;
    /* SAH cost of the BVH4 in force and of the tree as last built (pt_create or a rebuild): the
       sum over nodes (the root included) and leaves of the stored box's half area times 1 per node
       or 0.5 per leaf triangle (the collapse's constants), over the half area the root had when
       the tree was last built.  Both use that one divisor, so their ratio is the ratio of the plain
       area sums: a refit that stretches boxes raises it above 1 even when the scene box grows with
       them.  fp64 in a fixed order: the same node array always gives the same number. */
    double bvh_sah_cost;
    double bvh_sah_cost_built;
} pt_stats;

typedef struct pt_renderer pt_renderer;

/* OptixRenderer::OptixRenderer(ptxPath, Model*) — Renderer/OptiX/OptixRenderer.cpp:9-36.
 * Uploads the scene and builds the LBVH on the GPU (replaces BuildAccel, :306-456). */
int pt_create(const pt_scene* scene, const pt_options* options, pt_renderer** out);
/* no destructor in the reference (it leaks); frees every device buffer. */
int pt_destroy(pt_renderer* r);

/* OptixRenderer::Resize(glm::ivec2&) — OptixRenderer.cpp:649-660.  0-sized = no-op. */
int pt_resize(pt_renderer* r, int32_t width, int32_t height);
/* OptixRenderer::SetCamera(Camera*) — OptixRenderer.cpp:662-668: position + inverse view +
 * inverse projection, column-major glm::mat4. */
int pt_set_camera(pt_renderer* r, const float position[3], const float inverse_view[16],
                  const float inverse_projection[16]);
/* OptixRenderer::SetLights(std::vector<PointLight>*) — OptixRenderer.cpp:670-675 (re-settable). */
int pt_set_lights(pt_renderer* r, const pt_point_light* lights, int32_t count);
/* OptixRenderer::SetMaxBounces(int) — OptixRenderer.cpp:677-679.  0 renders black frames;
 * a negative count returns PT_ERR_INVALID. */
int pt_set_max_bounces(pt_renderer* r, int32_t max_bounces);
int pt_set_material_mode(pt_renderer* r, int32_t material_mode);
int pt_set_kernel(pt_renderer* r, int32_t kernel);
/* frames (spp) rendered per launch by pt_render_frames (default 128 since round 5; 64 before): the
   megakernel loops them in registers; the wavefront keeps all of their paths in flight in one
   kernel chain, at most 2^28 paths (128 frames at 1080p, 56 GB of queues per stream). */
int pt_set_frames_per_launch(pt_renderer* r, int32_t frames);
/* Upper bound on the device memory of the wavefront queues of all streams together (VERDICT
   round 5 item 6; the reference holds a 25 MB colour buffer, OptixRenderer.cpp:649-660, so a
   drop-in sharing the GPU with a viewer should not take a third of it).  bytes > 0: that many;
   0: the default, a quarter of the device memory (hipDeviceTotalMem / 4: on an MI355X the
   128-frame 1080p batch of one stream fits, two-stream Conductor / Dielectric calls take smaller
   batches); < 0: no
   budget (only the 2^28-path cap per stream).  A call lowers its frames per batch to fit (every
   batch size gives the same image) and frees queues that streams it does not use hold beyond
   the budget; pt_stats.queue_bytes reports what the queues hold. */
int pt_set_queue_budget(pt_renderer* r, int64_t bytes);
/* Tests only: while on, every speculative look-ahead batch (pt_set_render_ahead) starts with a
   kernel that waits until the batch is cancelled (a state change), the hold is switched off, or
   10 s pass, so a test can change the state while the batch is provably in flight. */
int pt_set_debug_hold(pt_renderer* r, int32_t on);
/* Diagnostics (counted while pt_set_traversal_stats is on, since pt_stats_reset): how coherent the
   wavefront trace kernels' global BVH node loads are.  For every wave step in which some lanes
   load a node from global memory (not from the LDS-staged top levels), the number of distinct
   nodes those lanes load: hist[0..5] = steps with 1, 2, 3-4, 5-8, 9-16, 17-64 distinct nodes,
   hist[6] = all such steps, hist[7] = the lanes that loaded a global node (VERDICT round 5
   item 5: a wave-uniform scalar-cache node fetch pays only if few distinct nodes are common).
   A multi-device renderer sums every device's counts. */
int pt_get_trace_coherence(pt_renderer* r, uint64_t hist[8]);
/* Diagnostics: count BVH nodes visited / triangle tests / rays (slower instrumented kernels). */
int pt_set_traversal_stats(pt_renderer* r, int32_t enable);
/* Bracket every wavefront trace launch (k_extend, k_trace_pair) with its own HIP event pair
 * on the library stream (pt_stats.trace_kernel_ms / trace_kernel_launches).  Off by default. */
int pt_set_kernel_timing(pt_renderer* r, int32_t enable);
/* Wavefront: the camera ray of a pixel is the same in every frame (no pixel jitter,
 * devicePrograms.cu:601-623), so a batch of frames traces it once per pixel and copies the
 * hit record to every frame (default 1).  0 traces every frame's copy; the images are
 * bit-identical either way. */
int pt_set_primary_dedup(pt_renderer* r, int32_t enable);
/* Wavefront: streams the batches of a pt_render_frames call alternate between (1 to 4, or 0 =
 * auto, the default since round 5: two for the Conductor and Dielectric modes, one otherwise; a
 * one-frame call in row bands takes two in every mode).  With more than 1, consecutive batches run on different
 * streams with their own queues, so one batch's kernels overlap another's; the batches still add
 * into the sum in frame order, and the image is bit-identical to 1.  A call uses at most as many
 * streams as it has batches.  Round 5: with the trace kernels' ray pools a second
 * stream no longer pays for Lambert (1537 vs 1508 Msamples/s at 128 frames), Default or Layered,
 * and still does for Dielectric (+4 %) and Conductor (+0.6 %). */
int pt_set_wavefront_streams(pt_renderer* r, int32_t streams);
/* Wavefront, a call of one frame (pt_render without render-ahead, pt_render_frames with n = 1,
 * pt_launch): with 2 or more wavefront streams, the frame's rows are split into two bands that
 * render on two streams at once, each band's kernels filling the other's SIMT tails (default 1).
 * Every pixel's path depends only on its pixel and frame id: the image is bit-identical to 0. */
int pt_set_band_split(pt_renderer* r, int32_t enable);
/* Wavefront: the lit table, one bit per (point light, surface cell) that is set only where every
 * NEE shadow ray from that cell toward that light is provably unoccluded (from the geometry and
 * the light positions alone, any camera, any bounce).  The shading kernels add such a light's
 * contribution at once instead of queueing a shadow ray; the images are bit-identical.  enable:
 * < 0 auto (the default: on in the Lambert, Default and Layered modes, where it measured faster;
 * off in Dielectric, which lost 1.2 %, in Conductor, not measured, and for pt_launch calls, whose
 * one frame cannot pay for a build), 0 off, > 0 on (also for pt_launch: rebuilt on every such
 * call, about 2 ms on a 35k-triangle scene, and again for the renderer's own lights afterwards).
 * The table is rebuilt on the library stream when the lights change (pt_set_lights); it is not
 * used with more than 16 lights, more than 2^23 cells or vertex coordinates beyond 128 units, and
 * a light beyond 128 units has no bits (its shadow rays are traced). */
int pt_set_lit_table(pt_renderer* r, int32_t enable);
/* Tests: the lit table for the current lights (built now if it is stale).  info is always written;
 * tri_words (one 32-bit word per leaf-ordered triangle: subdivision level << 24 | first cell, level
 * 255 = no cells) and bits (lights x words_per_light 32-bit words) are copied when not NULL and
 * their byte sizes match.  active = 0: no table (switched off, or one of the limits above). */
typedef struct pt_lit_table_info {
    int32_t active;
    int32_t lights;
    uint32_t triangles;
    uint32_t cells;
    uint32_t words_per_light;
    float delta;
    float margin; /* the largest margin a cell can have; each (light, cell) uses its own, smaller one */
} pt_lit_table_info;
int pt_lit_table_download(pt_renderer* r, pt_lit_table_info* info, uint32_t* tri_words, int64_t tri_bytes,
                          uint32_t* bits, int64_t bits_bytes);
/* The occluder candidate table: beside the lit table, one int32 per (light, cell), laid out
 * light * cells + cell, holding -1 or a leaf-order triangle that probably occludes the cell's shadow
 * rays (the closest hit of the ray from the cell's centroid).  Before a shading kernel emits a shadow
 * ray the lit table did not answer, it tests that one triangle with the tracer's own arithmetic on
 * the very ray; a hit is the tracer's answer "occluded" whatever triangle the entry names, so the
 * ray is dropped and images stay bit-identical.  A wrong entry only costs speed.  < 0: automatic
 * (the default: on in the Lambert, Default and Layered modes while pt_set_lit_table is in auto too;
 * a lit table forced on is measured alone), 0: off, > 0: on.  It needs the lit table in use and is
 * rebuilt with it (lights set, geometry committed).  Without the memory for it the renderer runs
 * without it. */
int pt_set_occluder_table(pt_renderer* r, int32_t enable);
/* Tests: the table for the current lights (built now if stale).  *entries_out = lights * cells, or
 * 0 while it is not in use; `entries` is filled when not NULL and `bytes` = 4 * *entries_out.
 * pt_occluder_table_upload replaces the entries until the next rebuild; an entry outside
 * [-1, triangles) is rejected with PT_ERR_INVALID and nothing is written. */
int pt_occluder_table_download(pt_renderer* r, int64_t* entries_out, int32_t* entries, int64_t bytes);
int pt_occluder_table_upload(pt_renderer* r, const int32_t* entries, int64_t bytes);
/* The skip table: two 32-bit words per leaf-order triangle, one for each side of the stored winding,
 * computed from the triangle records and the BVH alone.  A word is 0 or names the highest BVH4 child
 * link on the triangle's root-to-leaf path whose whole subtree lies at or below the triangle's plane
 * on that side.  The fused shading kernels (Lambert, Conductor, Dielectric) store the word with a
 * continuation ray that climbs from that side (dot(direction, offset direction) > 2^-6), and the
 * trace kernel drops the named subtree unvisited: no triangle in it can be hit, so images stay
 * bit-identical.  < 0: automatic (the default: on in the modes where it measured a gain), 0: off,
 * > 0: on.  Built with the scene and rebuilt by every geometry commit, on the library stream; not
 * used with vertex coordinates beyond 128 units, and without the memory for it the renderer runs
 * without it. */
int pt_set_skip_table(pt_renderer* r, int32_t enable);
/* Tests: the words for the tree in force (built now if stale).  *words_out = 2 * triangles, or 0 while
 * the table is not in use; `words` is filled when not NULL and `bytes` = 4 * *words_out. */
int pt_skip_table_download(pt_renderer* r, int64_t* words_out, uint32_t* words, int64_t bytes);

/* LaunchParams (Renderer/OptiX/LaunchParams.h:9-28) as a C struct: the state one optixLaunch
 * reads.  Same fields and meaning; device pointers where the reference holds device pointers
 * (colorBuffer and pointlights are CUDABuffer d_pointer()s, OptixRenderer.cpp:617-637,670-675);
 * `traversable` is replaced by the renderer's own BVH. */
typedef struct pt_launch_params {
    struct {
        float* color_buffer; /* device: size[0]*size[1] glm::vec3 (RGB fp32), row 0 = bottom */
        int32_t size[2];
        uint32_t id; /* seeds tea<16>(W*y+x, id) (devicePrograms.cu:631) */
    } frame;
    struct {
        float position[3];
        float inverse_view_matrix[16];       /* column-major (glm) */
        float inverse_projection_matrix[16]; /* column-major (glm) */
    } camera;
    const pt_point_light* point_lights; /* device array of point_light_count lights */
    int32_t point_light_count;
    int32_t max_bounces;
} pt_launch_params;

/* optixLaunch(pipeline, stream, launchParams, ..., size.x, size.y, 1) — OptixRenderer.cpp:627-637
 * running __raygen__renderFrame (devicePrograms.cu:666-706): every pixel's sample of frame.id is
 * written (not added) to frame.color_buffer.  Asynchronous on pt_stream(r); pt_synchronize waits
 * (the reference's CUDA_SYNC_CHECK).  The renderer's own size, camera, lights and max bounces are
 * not changed.  A zero size is a no-op; a negative max_bounces or count is PT_ERR_INVALID. */
int pt_launch(pt_renderer* r, const pt_launch_params* params);

/* ---- geometry updates on a live renderer -----------------------------------------------------
 * The reference bakes its scene once (BuildAccel, OptixRenderer.cpp:306-456); these calls move a
 * mesh without pt_destroy / pt_create: textures, queues, rings and every setting stay.  The two
 * setters only STAGE a change: rendering is not affected until pt_commit_geometry.  Topology,
 * texcoords and materials do not change.
 * Stage a new model matrix (column-major, as pt_mesh.model_matrix) for mesh `mesh`. */
int pt_set_mesh_transform(pt_renderer* r, int32_t mesh, const float model_matrix[16]);
/* Stage new object-space vertices (n_vertices*3, the count given at pt_create) and, if not NULL,
 * normals (n_vertices*3; NULL keeps the current ones).  PT_ERR_INVALID if normals are passed for a
 * mesh that was created without them. */
int pt_set_mesh_vertices(pt_renderer* r, int32_t mesh, const float* vertices, const float* normals);
#define PT_GEOM_REFIT 0   /* keep the tree's topology, recompute every node box */
#define PT_GEOM_REBUILD 1 /* rebuild with the builder chosen at pt_create */
/* Apply the staged changes on every device of the renderer.  Nothing staged: a no-op returning
 * PT_OK.  The commit cancels a speculative look-ahead batch (as a camera move does), waits for the
 * rendering already enqueued, re-bakes the changed meshes' triangle records on the device and
 * recomputes every BVH4 node box (both in place, bit-identical to what pt_create stores for the
 * moved scene and this topology); PT_GEOM_REBUILD then builds a new tree as pt_create would and
 * swaps it in.  SYNCHRONOUS in this version: it returns once the new geometry is in force (the lit
 * table's cells are re-cut on the host).  Images are bit-identical to a renderer created from the
 * moved scene, for a refit of any quality; pt_stats.bvh_sah_cost / bvh_sah_cost_built tells when a
 * rebuild pays.  No frame rendered ahead before the commit is served after it.  The lit table
 * follows: a vertex beyond 128 units switches it off, a later commit back inside switches it on.
 * A rebuild whose tree is too deep for the traversal stack returns PT_ERR_INVALID and leaves the
 * refitted tree (valid, with the new geometry) in force. */
int pt_commit_geometry(pt_renderer* r, int32_t how);

/* OptixRenderer::Render(glm::vec3 h_pixels[]) — OptixRenderer.cpp:617-647: frame.id++,
 * one sample per pixel, synchronous, downloads W*H*3 floats to host_rgb.  No-op before
 * the first pt_resize (as :621). */
int pt_render(pt_renderer* r, float* host_rgb);
/* Render-ahead for pt_render / pt_display_add_frame (wavefront kernel; default 64 frames, 1 = off).
 * While the size, camera, lights, max bounces, material mode and kernel stay the same between
 * calls, a call whose frame id is not ready renders the next k frame ids as one batch into a ring
 * of 1-spp images, k doubling on each such call that continues the sequence (1, 2, 4, ...) and
 * restarting at 1 after any change; later calls download their frame from the ring.  Once k
 * reaches its target, the first pt_render served from a batch also enqueues the following k frame
 * ids into a second ring, which the GPU renders while the caller downloads the current batch
 * (pt_render copies on a stream of its own).  The target is the smallest of `frames`, a memory
 * cap and a time budget: a batch's wavefront queues (208 B per path) and the two rings (2 * k
 * W*H*3 floats) take at most a quarter of the device memory and no more than is free, and a
 * batch's estimated duration (from the last measured ring batch) stays within
 * pt_set_render_ahead_budget (default 50 ms) -- the most a call that changes the state waits
 * for work already enqueued.  At 1080p 64 frames hold about 31 GB.  Every image is bit-identical
 * to rendering its frame alone.  A batch that does not fit in device memory lowers the cap for
 * the rest of the sequence, and the call renders its own frame alone.  With a debug pixel set
 * (pt_set_debug_pixel) every call renders its own frame, so the records belong to that call. */
int pt_set_render_ahead(pt_renderer* r, int32_t frames);
/* Upper bound, in ms of estimated GPU time, on one render-ahead batch (default 50; 0 = none). */
int pt_set_render_ahead_budget(pt_renderer* r, float max_ms);

/* Device-resident accumulation (replaces the per-spp download + GL blend of
 * Renderer/OptixView.cpp:201-255 / AddPathtracedFrame.frag:18-24).  Renders frame ids
 * first_frame_id .. first_frame_id+n_frames-1 and ADDS each sample's radiance, in frame
 * order, into the fp32 sum buffer.  Asynchronous on the library stream. */
int pt_accum_clear(pt_renderer* r);
int pt_render_frames(pt_renderer* r, uint32_t first_frame_id, uint32_t n_frames);
/* One call for a whole image (SURVEY §8(b) "pt_render_accumulate"): clear, render frame ids
 * first_frame_id .. first_frame_id+spp-1 into the sum buffer, then (if host_rgb_mean is not
 * NULL) download the mean, sum / spp, as the reference's running-mean display converges to
 * (OptixView.cpp:232-245 with maxSamples < 0).  Synchronous; the sum stays on the device. */
int pt_render_accumulate(pt_renderer* r, uint32_t spp, uint32_t first_frame_id, float* host_rgb_mean);
/* Use caller-owned device memory (W*H*3 floats) as the sum buffer (e.g. an RCCL buffer);
 * NULL reverts to the internal buffer. */
int pt_set_accum_device_buffer(pt_renderer* r, float* device_sum_rgb);
float* pt_accum_device_ptr(pt_renderer* r);
/* Download the sum (scale = 1) or the mean (scale = 1/spp) to host. */
int pt_accum_download(pt_renderer* r, float* host_rgb, float scale);
/* fp64 accumulation (off by default: the reference's sum is fp32, OptixView.cpp:232-245).  On:
 * every sample's fp32 radiance is added in fp64 and the fp32 sum buffer holds the fp64 sum
 * rounded to fp32; a multi-device renderer reduces the devices' fp64 sums (ncclFloat64), so the
 * image no longer depends on how the frame ids were split over devices (up to fp64 rounding,
 * ~1e-16 relative, which the final rounding to fp32 almost always absorbs).  Switching it on
 * starts from the current fp32 sum.  Wavefront kernel only (PT_KERNEL_AUTO resolves to it);
 * a megakernel render returns PT_ERR_INVALID. */
int pt_set_accum_fp64(pt_renderer* r, int32_t on);
double* pt_accum_device_ptr64(pt_renderer* r);  /* NULL while off */
int pt_accum_download64(pt_renderer* r, double* host_rgb);

/* Waits for every device of the renderer. */
int pt_synchronize(pt_renderer* r);
/* hipStream_t of the library (of device_list[0]).  After pt_render returns, a look-ahead batch
 * (pt_set_render_ahead) may still be running on it: work a caller enqueues on this stream runs
 * after that batch; pt_synchronize waits for it. */
void* pt_stream(pt_renderer* r);
/* Devices of a multi-device renderer (1 for a single-device one); ordinals into devices[]
 * (at most max entries). */
int32_t pt_device_count(const pt_renderer* r);
int pt_devices(const pt_renderer* r, int32_t* devices, int32_t max);
uint32_t pt_frame_id(const pt_renderer* r);
int pt_set_frame_id(pt_renderer* r, uint32_t frame_id);
int pt_get_stats(pt_renderer* r, pt_stats* out);
int pt_stats_reset(pt_renderer* r);

/* Camera helper: Renderer/Camera.cpp:6-70 + GlmHelperMethods.cpp:4-10 (Blender position /
 * rotation in degrees -> engine position, inverse view, inverse projection for the given
 * frame size; "horizontal" FOV used as fovy, as the reference does). */
int pt_camera_from_blender(const float blender_position[3], const float blender_rotation_deg[3],
                           float fov_deg, int32_t width, int32_t height, float position[3],
                           float inverse_view[16], float inverse_projection[16]);

/* Debug / parity: trace n rays (origin xyz, dir xyz, tmin, tmax per ray = 8 floats) against
 * the renderer's BVH, whichever builder made it, with the per-lane traversal kernel (k_trace).
 * prim = global triangle index (meshes concatenated) or -1. */
int pt_trace_rays(pt_renderer* r, const float* host_rays, int32_t n, int32_t* prim, float* t,
                  float* u, float* v, int32_t* backface, int32_t any_hit);

/* Debug path: the reference's isDebugRay (devicePrograms.cu:637-644, printed at :428-437) as
 * data.  While set, the path of pixel (x, y) (row 0 = bottom) at frame frame_id records every
 * bounce it shades -- in whichever render call covers that frame, on device_list[0] -- and
 * pt_get_debug_path downloads the records (at most max; *n_bounces = how many were recorded).
 * x < 0 turns it off.  The CPU oracle records the same fields (oracle orc_sample_path_debug). */
typedef struct pt_debug_bounce {
    int32_t bounce;             /* rayData->bounceCounter after the hit (devicePrograms.cu:360), 1.. */
    int32_t prim;               /* global triangle index of the hit */
    float position[3];          /* surface.position */
    float albedo[3];            /* surface.albedo (after SampleTextures) */
    float shading_normal[3];    /* surface.sNormal (face-forwarded, back-face flipped, normal-mapped) */
    float geometry_normal[3];   /* surface.gNormal */
    float roughness, metallic;
    float beta[3];              /* path throughput entering the bounce */
    float radiance[3];          /* path radiance gathered before the bounce's NEE */
} pt_debug_bounce;
int pt_set_debug_pixel(pt_renderer* r, int32_t x, int32_t y, uint32_t frame_id);
int pt_get_debug_path(pt_renderer* r, pt_debug_bounce* out, int32_t max, int32_t* n_bounces);

/* Debug / determinism: copy the BVH4 node array (128 B per node, pt_stats.bvh_nodes nodes) and
 * the leaf-ordered triangle records (48 B per triangle) to host; at most the given byte counts. */
int pt_bvh_download(pt_renderer* r, void* nodes, int64_t node_bytes, void* triangles, int64_t triangle_bytes);

const char* pt_last_error(void);
const char* pt_version(void);

/* ---- headless progressive view --------------------------------
 * OptixView::AddNewFrameToBuffer (Renderer/OptixView.cpp:226-255) + AddPathtracedFrame.frag
 * :18-24 on the device.  pt_display_reset clears the view buffer to 1.0 (glClearColor(1,1,1,1),
 * OptixView.cpp:145-149) and sets maxSamples; each pt_display_add_frame renders one spp like
 * pt_render (frame.id++) and blends it: max_samples < 0 -> fb = mix(fb, new, 1/n) (running
 * mean), else fb += new * (1/max_samples).  *samples (optional) receives n. */
int pt_display_reset(pt_renderer* r, int32_t max_samples);
int pt_display_add_frame(pt_renderer* r, int32_t* samples);
int pt_display_download(pt_renderer* r, float* rgb);

/* ---- first-hit feature buffers (AOVs) and the denoiser ----------------------
 * The G-buffer: per pixel of the renderer's size, camera and committed geometry, the surface the
 * pixel-centre camera ray hits first -- traced over the radiance ray's interval [0, 100] with its
 * strict re-trace rule and alpha cut-out, reconstructed as the first bounce of a path is.  It does
 * not depend on the frame id, the lights or the material mode.  Rows as the colour buffer (row 0 =
 * bottom); a miss holds prim = -1 and 0 in every float.  It is rendered on first use and cached:
 * only a new size, camera or geometry commit renders it again (pt_denoise_info.gbuffer_renders).
 * Everything here runs on the library stream of device_list[0], so a call orders itself after the
 * accumulation or display work already enqueued; it also waits behind a look-ahead batch in flight
 * (pt_set_render_ahead). */
#define PT_AOV_ALBEDO 0       /* float x 3: surface.albedo, after the textures */
#define PT_AOV_NORMAL 1       /* float x 3: the shading normal (normal-mapped, face-forwarded) */
#define PT_AOV_GEOM_NORMAL 2  /* float x 3: the geometric normal */
#define PT_AOV_POSITION 3     /* float x 3 */
#define PT_AOV_DEPTH 4        /* float x 1: the hit distance along the camera ray */
#define PT_AOV_PRIM 5         /* int32 x 1: global triangle index, as pt_trace_rays reports it */
#define PT_AOV_ROUGH_METAL 6  /* float x 2: roughness, metallic */
/* Channels of one AOV (3, 3, 3, 3, 1, 1, 2); < 0 for a kind that does not exist. */
int pt_aov_channels(int32_t kind);
/* Renders the G-buffer if it is stale and copies one AOV to host; bytes must be W * H * channels * 4. */
int pt_aov_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes);
/* The AOV on the device (W * H * channels elements); NULL until the G-buffer was first rendered.  It
 * holds the view of the last render: pt_aov_download or pt_denoise bring it up to date. */
const void* pt_aov_device_ptr(pt_renderer* r, int32_t kind);

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the G-buffer's normal and
 * position, on albedo-demodulated colour.  Every struct here leads with struct_size = the sizeof the
 * caller compiled against: the library reads and writes min(struct_size, its own sizeof) bytes, and
 * fields a shorter caller does not have take their defaults. */
typedef struct pt_denoise_options {
    uint32_t struct_size;
    int32_t iterations;    /* 1..8; iteration i taps at a spacing of 2^i pixels */
    int32_t demodulate;    /* != 0: filter colour / max(albedo, albedo_floor), multiply back afterwards */
    float sigma_color;     /* halved per iteration */
    float sigma_normal;
    float sigma_position;
    float albedo_floor;
} pt_denoise_options;
/* Fills the defaults (5, 1, 1.0, 0.3, 1.0, 1e-3) into the first o->struct_size bytes. */
int pt_denoise_options_default(pt_denoise_options* o);
#define PT_DENOISE_SRC_ACCUM 0   /* the sum buffer: with scale = 1/spp the values pt_accum_download gives */
#define PT_DENOISE_SRC_DISPLAY 1 /* the pt_display_* buffer; PT_ERR_STATE before pt_display_reset */
#define PT_DENOISE_SRC_HOST 2    /* host_in, W*H*3 floats */
/* Filters source * scale (opt NULL = the defaults) into a device buffer of W*H*3 floats and, unless
 * host_out is NULL, downloads it.  Miss pixels come back as they went in.  Asynchronous without
 * host_out (except for the upload of a host source).  PT_ERR_INVALID for a bad source, iterations
 * outside 1..8, or a sigma or floor that is not > 0; PT_ERR_STATE before the first pt_resize. */
int pt_denoise(pt_renderer* r, int32_t source, const float* host_in, float scale, const pt_denoise_options* opt,
               float* host_out);
/* The last pt_denoise result on the device (W*H*3 floats); NULL before the first. */
float* pt_denoised_device_ptr(pt_renderer* r);
typedef struct pt_denoise_info {
    uint32_t struct_size;
    int32_t iterations;       /* of the last pt_denoise */
    uint64_t gbuffer_renders; /* G-buffer renders since pt_create */
    uint64_t hit_pixels;      /* pixels of the current G-buffer whose camera ray hits */
    double gbuffer_ms;        /* HIP-event time of the last G-buffer render */
    double filter_ms;         /* HIP-event time of the last pt_denoise's kernels (its G-buffer render excluded) */
} pt_denoise_info;
/* Waits for the library stream. */
int pt_get_denoise_info(pt_renderer* r, pt_denoise_info* out);

/* ---- temporal reprojection and the variance-guided filter --------------------
 * SVGF (Schied et al. 2017) on top of pt_denoise: a call reprojects the previous call's filtered
 * colour, luminance moments and history length through the previous call's camera, accepts them
 * per pixel where the previous guides show the same surface, blends this call's source into them,
 * and runs the a-trous iterations with a colour term scaled by the estimated variance.  A camera
 * or committed geometry change therefore keeps the samples of the surfaces still in view.  By
 * default a point on a moved mesh fails the plane test and starts again; with motion_vectors on it
 * is followed to where it was (below).  Same device, stream and ordering as pt_denoise. */
typedef struct pt_temporal_options {
    uint32_t struct_size;
    float alpha;              /* (0, 1]: the share of the new colour; at least 1 / history length */
    float alpha_moments;      /* (0, 1]: likewise for the luminance moments */
    int32_t max_history;      /* >= 1: the history length stops growing here */
    float normal_cos;         /* [-1, 1]: a tap is accepted if dot(n_prev, n) >= normal_cos */
    float plane_distance;     /* > 0: ... and |dot(pos - pos_prev, n)| <= plane_distance * depth */
    float sigma_luminance;    /* > 0: the colour term is |dl| / (sigma_luminance * sqrt(variance) + 1e-8) */
    int32_t variance_history; /* >= 0: below this history length the variance is estimated spatially (7x7) */
    int32_t motion_vectors;   /* != 0: reproject a hit point from where it was on its triangle at the previous call */
} pt_temporal_options;
/* Fills the defaults (0.2, 0.2, 32, 0.9, 0.02, 4.0, 4, 0) into the first o->struct_size bytes. */
int pt_temporal_options_default(pt_temporal_options* o);
/* As pt_denoise (sources, scale, NULL = defaults, host_out, asynchrony), with the history of the
 * previous call; this call's view and filtered state become the history of the next.  dopt gives
 * iterations, demodulate, sigma_normal, sigma_position and albedo_floor; its sigma_color is not
 * used.  The result is where pt_denoised_device_ptr points.  PT_ERR_INVALID for what pt_denoise
 * refuses and for a temporal option outside the range given above. */
int pt_denoise_temporal(pt_renderer* r, int32_t source, const float* host_in, float scale, const pt_temporal_options* topt,
                        const pt_denoise_options* dopt, float* host_out);
/* Drops the history: the next call starts every pixel again.  pt_resize does the same. */
int pt_temporal_reset(pt_renderer* r);
#define PT_TEMPORAL_HISTORY_LENGTH 0 /* float x 1: 0 at a miss, 1 where the history was not accepted */
#define PT_TEMPORAL_MOMENTS 1        /* float x 2: first and second moment of the luminance */
#define PT_TEMPORAL_VARIANCE 2       /* float x 1: the variance that entered iteration 0 */
#define PT_TEMPORAL_COLOR 3          /* float x 3: the stored colour history (iteration 0's result, demodulated) */
/* Channels of a PT_TEMPORAL_* kind; -1 for an unknown kind. */
int pt_temporal_channels(int32_t kind);
/* Copies state of the last pt_denoise_temporal to host; bytes must be W * H * channels * 4.
 * PT_ERR_STATE before the first call (or after a pt_resize). */
int pt_temporal_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes);
typedef struct pt_temporal_info {
    uint32_t struct_size;
    int32_t history_valid;       /* != 0: the next call has a history to reproject into */
    uint64_t calls;              /* pt_denoise_temporal calls since pt_create */
    uint64_t reprojected_pixels; /* hit pixels of the last call with accepted history */
    uint64_t reset_pixels;       /* hit pixels of the last call without */
    double temporal_ms;          /* HIP-event times of the last call: pack, reproject and blend */
    double variance_ms;          /* the spatial variance estimate */
    double filter_ms;            /* the iterations with their divisor passes, and keeping the guides */
    uint64_t moved_pixels;       /* hit pixels of the last call whose previous position differs from the present one */
    double snapshot_ms;          /* HIP-event time of the last call's vertex snapshot; 0 if none ran */
    int32_t motion_used;         /* 1 iff the motion kernel ran in the last call */
    int32_t reserved;
} pt_temporal_info;
/* Waits for the library stream. */
int pt_get_temporal_info(pt_renderer* r, pt_temporal_info* out);

/* Motion vectors.  With pt_temporal_options.motion_vectors != 0 a call ends by
 * keeping the world-space vertices of every triangle (one copy kernel, only when the geometry was
 * committed since the copy was made).  The next such call, if geometry was committed in between,
 * reprojects each hit pixel from pp = its barycentrics applied to its triangle's kept vertices --
 * where that point of the surface was -- instead of from its present position; pp goes through the
 * previous camera and into the plane test, everything else is as without the option.  Rigid moves
 * and vertex deformation alike; several commits between two calls are one move.  A call whose
 * predecessor did not have the option on, or that has no history, runs as without it and keeps the
 * vertices for the next.  Off by default: a surface's irradiance is anchored to the static lights,
 * not to the surface, so history followed across a move that changes the lighting is stale (measured
 * in DESIGN.md §11). */
#define PT_MOTION_BARYCENTRIC 0   /* float x 2: u, v of the G-buffer in force (rendered if stale, as pt_aov_download) */
#define PT_MOTION_PREV_POSITION 1 /* float x 3: pp of the last pt_denoise_temporal with motion_vectors on; where that
                                     call ran the plain kernel, the position guide itself; 0 at a miss */
#define PT_MOTION_SCREEN 2        /* float x 3: (fx - x, fy - y, 1) in pixels for a hit pixel of a call that had a history
                                     and clip.w > 0, with fx, fy of §11 step 1 from pp; else (0, 0, 0) */
/* Channels of a PT_MOTION_* kind (2, 3, 3); < 0 for a kind that does not exist. */
int pt_motion_channels(int32_t kind);
/* Copies one of them to host; bytes must be W * H * channels * 4.  Kinds 1 and 2: PT_ERR_STATE unless
 * the last pt_denoise_temporal had motion_vectors on. */
int pt_motion_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes);

/* ---- adaptive sampling ---------------------------------------------------
 * pt_render_adaptive renders rounds of round_frames frames, each only for the pixels of the 8x8
 * tiles (aligned to pixel (0, 0) at the bottom-left, clipped at the right and top edges) that have
 * not stopped.  Per pixel it keeps the sample count n, the fp32 RGB sum (the accumulation buffer)
 * and the fp64 sums S1, S2 of the samples' luminance Y = (0.2126 r + 0.7152 g) + 0.0722 b (fp32)
 * and of Y * Y.  After a round, in fp64: m = S1 / n, v = max(S2 / n - m * m, 0) / n,
 * e = sqrt(v) / max(m, luminance_floor) (max(a, b) = a < b ? b : a, so a NaN stays); a tile's
 * error is the pairwise-tree sum of e over its pixels divided by their number.  A tile stops, for
 * good, once its error <= threshold and its pixels hold >= min_samples samples; every tile stops at
 * max_samples.  A pixel therefore holds the samples of frame ids first .. first + n - 1, added in
 * frame order: its sum is bit for bit what pt_render_frames(first, n) leaves there.  Wavefront
 * kernel, one device, fp32 accumulation into the library's own buffer; no band split. */
typedef struct pt_adaptive_options {
    uint32_t struct_size;
    float threshold;       /* > 0 or == 0: mean relative standard error of a tile's pixels at which it stops */
    int32_t min_samples;   /* >= 1, rounded up to a multiple of round_frames */
    int32_t max_samples;   /* >= min_samples, rounded up likewise */
    int32_t round_frames;  /* >= 2 */
    float luminance_floor; /* > 0 */
} pt_adaptive_options;
/* Fills the defaults (0.05, 16, 1024, 16, 0.01) into the first o->struct_size bytes. */
int pt_adaptive_options_default(pt_adaptive_options* o);
/* Clears the sum (as pt_render_accumulate) and the adaptive state, renders until no tile is active,
 * and, unless host_rgb_mean is NULL, downloads the per-pixel mean sum / n (W*H*3 floats).
 * Synchronous: the host reads the active-pixel count after every round.  opt NULL = the defaults.
 * PT_ERR_INVALID for an option outside the range given above, the megakernel (PT_KERNEL_MEGA), a
 * multi-device renderer, pt_set_accum_fp64 on, a caller-owned accumulation buffer
 * (pt_set_accum_device_buffer) or a debug pixel set; PT_ERR_STATE before the first pt_resize. */
int pt_render_adaptive(pt_renderer* r, uint32_t first_frame_id, const pt_adaptive_options* opt, float* host_rgb_mean);
#define PT_ADAPTIVE_SAMPLES 0     /* uint32 x 1 per pixel */
#define PT_ADAPTIVE_ERROR 1       /* float x 1 per pixel: e of the last estimate the pixel took part in */
#define PT_ADAPTIVE_MOMENTS 2     /* double x 2 per pixel: S1, S2 */
#define PT_ADAPTIVE_TILE_ERROR 3  /* float x 1 per tile, tiles row-major from the bottom-left */
#define PT_ADAPTIVE_TILE_ROUNDS 4 /* int32 x 1 per tile: rounds the tile was rendered in */
/* Channels of a PT_ADAPTIVE_* kind (1, 1, 2, 1, 1); < 0 for a kind that does not exist. */
int pt_adaptive_channels(int32_t kind);
/* Copies state of the last pt_render_adaptive to host; bytes must be elements * channels * the
 * element size above, with W * H elements for the per-pixel kinds and ceil(W / 8) * ceil(H / 8) for
 * the per-tile ones.  PT_ERR_STATE without such a call since the last pt_resize or pt_accum_clear. */
int pt_adaptive_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes);
/* The per-pixel mean of the last pt_render_adaptive on the device (W*H*3 floats); NULL without one. */
float* pt_adaptive_mean_device_ptr(pt_renderer* r);
typedef struct pt_adaptive_info {
    uint32_t struct_size;
    int32_t rounds;           /* of the last pt_render_adaptive */
    int32_t tiles;
    int32_t tiles_stopped;    /* tiles that met the threshold (the others ran to max_samples) */
    uint64_t samples;         /* the sum of n over the pixels */
    uint64_t samples_uniform; /* W * H * the largest n: what the same worst-case count costs on every pixel */
    double render_ms;         /* wall time of the rounds' rendering, their waits included */
    double estimate_ms;       /* HIP-event time of the error, compaction and resolve kernels */
} pt_adaptive_info;
/* Of the last pt_render_adaptive; zeros (and tiles of the present size) without one. */
int pt_get_adaptive_info(pt_renderer* r, pt_adaptive_info* out);
#define PT_DENOISE_SRC_ADAPTIVE 3 /* pt_denoise / pt_denoise_temporal source: the per-pixel mean of the last
                                     pt_render_adaptive; PT_ERR_STATE without one, PT_ERR_INVALID unless
                                     host_in is NULL */

/* ---- anti-aliasing: sub-pixel sampling and the pixel filter ----------------
 * With supersample = s in {2, 4, 8}, output pixel (x, y) at frame F takes the path of pixel
 * (s x + sx, s y + sy) of an image s times as large each way under the same camera, at frame F: its
 * camera ray and its seed tea16(sW y' + x', F).  The cell (sx, sy) depends on F alone: with c =
 * F mod s^2 and b = log2 s, sx is the top b bits of the 32-bit radical inverse of c and sy the top
 * b bits of the second Sobol' dimension of c (direction numbers v0 = 2^31, v(k+1) = v(k) ^ (v(k) >> 1)),
 * a permutation of the s^2 cells of which every aligned run of 4^k cell indices puts one sample in
 * each cell of the 2^k x 2^k coarsening.  A frame still costs W * H paths.
 * The sample of frame F sits at (ox, oy) = ((sx + 1/2) / s - 1/2, (sy + 1/2) / s - 1/2) from its
 * pixel's centre.  A filter of 1-D profile f and radius r (in output pixels) has R = ceil(r - 1/2)
 * in {0, 1, 2} and, per cell, the taps wx[i] = f(i + ox), i = -R..R, computed in fp64, divided by
 * their sum and rounded to fp32; wy likewise from oy.  The filtered image of one frame is, in fp32
 * without contraction,  g = 0;  for j = -R..R: for i = -R..R:
 *     g = g + (wy[j] * wx[i]) * L_F(clamp(X + i, 0, W - 1), clamp(Y + j, 0, H - 1))
 * (every tap is evaluated, so a sample that is not finite reaches its whole footprint), and the sum
 * buffer stays "the sum of the n frames' images", added in frame order.  R = 0 is the plain sum.
 *   f(t):  box       |t| <= r ? 1 : 0                                  (default r 0.5)
 *          tent      max(0, 1 - |t| / r)                               (default r 1.0)
 *          gaussian  max(0, exp(-t^2 / 2 sigma^2) - exp(-r^2 / 2 sigma^2)), sigma = param (default
 *                    0.5)                                              (default r 1.5)
 *          mitchell  Mitchell-Netravali at 2 t / r, B = param (default 1/3), C = (1 - B) / 2
 *                                                                      (default r 2.0)
 * The first-hit feature buffers (pt_aov_*) and with them the denoisers' guides stay at the pixel
 * centre, whatever the setting.  Wavefront kernel, one device.  With supersample > 1 the primary
 * dedup (pt_set_primary_dedup) is off: the frames of a batch no longer share their camera rays. */
#define PT_FILTER_BOX 0
#define PT_FILTER_TENT 1
#define PT_FILTER_GAUSSIAN 2
#define PT_FILTER_MITCHELL 3
typedef struct pt_pixel_filter {
    uint32_t struct_size;
    int32_t supersample; /* 1 (off), 2, 4 or 8 */
    int32_t kind;        /* PT_FILTER_* */
    float radius;        /* 0 = the kind's default; else 0.5 <= radius <= 2.5 */
    float param;         /* 0 = the kind's default; gaussian: sigma, mitchell: B */
} pt_pixel_filter;
/* Fills the defaults (1, PT_FILTER_BOX, 0, 0) into the first f->struct_size bytes. */
int pt_pixel_filter_default(pt_pixel_filter* f);
/* f NULL = the default.  Cancels a look-ahead batch in flight, as a camera change does; does not
 * clear the sum.  PT_ERR_INVALID for a supersample, kind or radius outside the above, taps whose
 * sum is not finite and positive, a multi-device renderer, or s^2 * W * H >= 2^31 (pt_resize refuses
 * such a size likewise while a filter is set).  While a setting other than the default is in force,
 * the render calls return PT_ERR_INVALID under the megakernel (PT_KERNEL_MEGA), and
 * pt_render_adaptive does with R > 0 (supersample > 1 under the box is allowed).  A one-frame call
 * with R > 0 does not split into row bands. */
int pt_set_pixel_filter(pt_renderer* r, const pt_pixel_filter* f);
/* The setting in force, radius and param resolved to the values in use. */
int pt_get_pixel_filter(pt_renderer* r, pt_pixel_filter* f);
/* Host only: xy[2 c], xy[2 c + 1] = (sx, sy) of cell index c, for c < supersample^2. */
int pt_pixel_filter_cells(int32_t supersample, int32_t* xy);
/* Host only: R of the filter and the 2 R + 1 taps along x and along y of cell index `cell`, exactly
 * the words the device reads (wx, wy: room for 5 floats each; any of R, wx, wy may be NULL). */
int pt_pixel_filter_taps(const pt_pixel_filter* f, int32_t cell, int32_t* R, float* wx, float* wy);

/* ---- glTF scene loading -----------------------------------------
 * ModelLoader::LoadModel (ModelLoading/ModelLoader.cpp:10-244): glTF 2.0 (.gltf with external
 * or data-URI buffers, or .glb) -> an owned pt_scene for pt_create.  One mesh per triangle
 * primitive, node transforms T*R*S composed down the hierarchy, baseColor / metallic /
 * roughness factors and texture ids, textures as RGBA8.  PNG is decoded internally; other
 * image formats (JPEG, ...; stb_image in the reference) go through `decode`, which is called
 * with rgba_out = NULL for the size and then with a width*height*4-byte buffer, and returns
 * 0 on success.  Deviations from the reference loader's bugs are listed in pt_gltf.cpp. */
typedef struct pt_model pt_model;
typedef int (*pt_image_decode_fn)(const uint8_t* data, size_t size, int32_t* width, int32_t* height,
                                  uint8_t* rgba_out, void* user);
int pt_model_load_gltf(const char* path, pt_image_decode_fn decode, void* user, pt_model** out);
const pt_scene* pt_model_scene(const pt_model* m);
const char* pt_model_mesh_name(const pt_model* m, int32_t index);
int pt_model_destroy(pt_model* m);
const char* pt_model_last_error(void);
/* The loader's PNG decoder (RGBA8, rows as stored); rgba_out = NULL returns the size. */
int pt_image_decode_png(const uint8_t* data, size_t size, int32_t* width, int32_t* height, uint8_t* rgba_out);

/* ---- image output and the parity metric ----------------------
 * Renderer/Images/WriteImage.cpp:35-99 (WriteEXR): float32 B,G,R scanline EXR, uncompressed,
 * rows flipped (rgb row 0 = bottom, as colorBuffer), a pixel with a NaN channel written as 0. */
int pt_image_write_exr(const char* path, const float* rgb, int32_t width, int32_t height);
/* WriteImage.cpp:8-32 (WriteBMP): clamp(v, 0, 1) * 255 truncated, 24-bit BMP. */
int pt_image_write_bmp(const char* path, const float* rgb, int32_t width, int32_t height);
/* Little-endian colour PFM, bottom row first. */
int pt_image_write_pfm(const char* path, const float* rgb, int32_t width, int32_t height);
/* Reads an uncompressed scanline EXR (half or float R,G,B) or a colour PFM into rgb (row 0 =
 * bottom).  rgb = NULL only returns the size. */
int pt_image_read(const char* path, float* rgb, int32_t* width, int32_t* height);
/* Per-image parity metric of SURVEY.md §8(c): mean over pixels x 3 channels of (a - b)^2,
 * pixels with a NaN channel counted as 0 (as the reference's EXR writer stores them). */
double pt_image_mse(const float* a, const float* b, int64_t n_pixels);
/* LDR-FLIP (Andersson et al. 2020; the README's second metric, README.md:42-46) of two linear
 * RGB images, each clamped to [0,1] and sRGB-encoded first.  pixels_per_degree <= 0 selects
 * 67 (0.7 m from a 0.7 m wide 3840-px display).  Returns the mean; error_map (optional)
 * receives the per-pixel values.  Algorithm notes in pt_image.cpp. */
double pt_image_flip(const float* ref, const float* test, int32_t width, int32_t height, float pixels_per_degree,
                     float* error_map);
const char* pt_image_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PTAMD_H */
