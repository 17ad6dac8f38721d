/*
 * psdr_hip.h -- C ABI of the MI355X-native differentiable wavefront renderer.
 *
 * This is the drop-in boundary for the hot path of uci-rendering/psdr-cuda
 * (Integrator.renderC / renderD and everything below it).  The reference has
 * no C ABI of its own: its boundary is the pybind11 module `psdr_cuda`
 * (reference src/psdr.cpp:40-295).  Every entry point below names the
 * reference interface it replaces (file:line relative to the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, non-zero on failure;
 *     psdr_last_error() returns the message (the reference throws
 *     psdr::Exception : std::runtime_error, include/misc/Exception.h:86-132).
 *   - all table pointers are CALLER-OWNED.  For libpsdr_hip.so they are
 *     DEVICE pointers (HBM); for the CPU oracle (oracle/psdr_oracle.cpp, test
 *     infrastructure only) the same structs carry HOST pointers.
 *   - float = IEEE fp32, indices = int32, images are interleaved RGB
 *     [H*W][3], pixel i = y*W + x, row 0 = top (reference
 *     src/integrator/integrator.cpp:76-88, docs/python_render.rst).
 *
 * The AD graph of the reference (Enoki DiffArray) is cut at the "scene
 * tables" built by Scene::configure (reference src/scene/scene.cpp:56-278):
 * kernels consume the tables (+ tangent tables in forward mode) and produce
 * the image (+ derivative image), or consume an adjoint image and scatter-add
 * into gradient tables (reverse mode).
 */
#ifndef PSDR_HIP_H
#define PSDR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- table strides (in 4-byte words) ------------------------------------ */
#define PSDR_TRI_STRIDE   24 /* p0 e1 e2 n0 n1 n2 face_normal (7x3) face_area, 2 pad
                                = TriangleInfo_, include/psdr/types.h:135-146 */
#define PSDR_TRIUV_STRIDE  8 /* uv0 uv1 uv2 (3x2), 2 pad = TriangleUV, types.h:154-155 */
#define PSDR_SEDGE_STRIDE 16 /* p0 e1 n0 n1 p2 (5x3) is_boundary(0/1)
                                = SecondaryEdgeInfo_, include/psdr/edge/edge.h:49-65 */
#define PSDR_PEDGE_STRIDE  8 /* p0(2) p1(2) edge_normal(2) edge_length, 1 pad
                                = PrimaryEdgeInfo_, edge.h:27-40 */
#define PSDR_BSDF_STRIDE  16 /* int32: type, then 5 x (texel offset, width, height) */
#define PSDR_EMITTER_F_STRIDE 8 /* radiance rgb, sampling_weight (normalised),
                                   inv_total_area, face pmf sum, 2 pad
                                   (src/emitter/area.cpp:10-62, src/shape/mesh.cpp:239-249) */
#define PSDR_EMITTER_I_STRIDE 4 /* mesh id, first global tri id, num faces, offset into face_cmf/pmf */
#define PSDR_CAM_WORDS    64 /* see below */
#define PSDR_ENV_WORDS    32 /* EnvironmentMap record (src/emitter/envmap.cpp:10-143,
                                include/psdr/emitter/envmap.h:38-46), see PSDR_ENV_* below */

/* tri_mesh[t] = mesh id | PSDR_TRI_FACE_NORMALS if the mesh uses face normals
   (scene.cpp:205-216 m_triangle_face_normals) */
#define PSDR_TRI_FACE_NORMALS 0x40000000

/* BSDF types (src/bsdf/diffuse.cpp, src/bsdf/roughconductor.cpp) */
#define PSDR_BSDF_DIFFUSE        0
#define PSDR_BSDF_ROUGHCONDUCTOR 1
/* MicrofacetBSDF (build-defined, DESIGN.md section 14, csrc/psdr_colloc_microfacet.h): Lambertian diffuse + isotropic GGX specular with a Schlick
   Fresnel term.  Evaluated by PSDR_INTEGRATOR_COLLOCATED only: every other integrator that evaluates a BSDF returns an error on a scene that
   announces this type. */
#define PSDR_BSDF_MICROFACET     2
/* MicrofacetBSDF with a tangent-space normal map (build-defined): the record of PSDR_BSDF_MICROFACET plus the map's
   (offset, width, height) in PSDR_SLOT_K -- 3 channels, image encoding: texel c decodes to v = 2c - 1, (0.5, 0.5, 1) is "no perturbation".  The lobes
   are evaluated about n' = normalize(s' v.x + t' v.y + n v.z): n the shading normal, s' the direction of increasing u on the triangle (from its three
   tri_uv rows) made orthogonal to n, t' = n x s'.  Needs tri_uv: the render entry points return an error for a scene that announces the type and has
   none.  Served like PSDR_BSDF_MICROFACET: PSDR_INTEGRATOR_COLLOCATED only. */
#define PSDR_BSDF_MICROFACET_NORMAL 3
/* MicrofacetBSDF with a height map (build-defined): the record of PSDR_BSDF_MICROFACET plus a 1-channel height map's
   (offset, width, height) in PSDR_SLOT_K and its scale's (offset, 1, 1) in PSDR_SLOT_ALPHA_V -- one texel, world length per unit of height.  The
   lobes are evaluated about n' = normalize(n - scale (h_u g_u + h_v g_v)): (h_u, h_v) the exact gradient of the bilinear map at the hit's uv,
   (g_u, g_v) the dual basis in the shading plane of the triangle's derivatives along u and v (from its three tri_uv rows).  Needs tri_uv like
   PSDR_BSDF_MICROFACET_NORMAL ("a height map needs texture coordinates") and is served like it: PSDR_INTEGRATOR_COLLOCATED only.  A record carries
   a normal map or a height map, never both. */
#define PSDR_BSDF_MICROFACET_HEIGHT 4
/* bsdf_rec parameter slots: slot s occupies words 1+3*s .. 3+3*s */
#define PSDR_SLOT_REFLECTANCE 0 /* Diffuse::m_reflectance / RoughConductor::m_specular_reflectance (3 ch) */
#define PSDR_SLOT_ALPHA_U     1 /* 1 ch */
#define PSDR_SLOT_ALPHA_V     2 /* 1 ch */
#define PSDR_SLOT_ETA         3 /* 3 ch */
#define PSDR_SLOT_K           4 /* 3 ch */
/* PSDR_BSDF_MICROFACET keeps the record's stride and reads three of its slots:
     PSDR_SLOT_REFLECTANCE  diffuse_reflectance kd (3 ch)
     PSDR_SLOT_ALPHA_U      roughness r (1 ch); the GGX width is alpha = r^2 in both directions
     PSDR_SLOT_ETA          specular_reflectance F0 (3 ch)
   PSDR_SLOT_ALPHA_V and PSDR_SLOT_K are unused and hold (offset, width, height) = (0, 1, 1).
   PSDR_BSDF_MICROFACET_NORMAL reads the same three and
     PSDR_SLOT_K            normal_map (3 ch)
   PSDR_BSDF_MICROFACET_HEIGHT reads the same three and
     PSDR_SLOT_K            height_map (1 ch)
     PSDR_SLOT_ALPHA_V      height_scale (1 ch, 1 x 1) */

/* cam[] layout (PerspectiveCamera, src/sensor/perspective.cpp:11-33), row-major 4x4 */
#define PSDR_CAM_SAMPLE_TO_CAMERA  0
#define PSDR_CAM_TO_WORLD         16
#define PSDR_CAM_WORLD_TO_SAMPLE  32
#define PSDR_CAM_POS              48
#define PSDR_CAM_DIR              51
#define PSDR_CAM_INV_AREA         54

/* env_f[] layout (EnvironmentMap): m_from_world and m_to_world as row-major 3x3 blocks (only
   transform_dir is ever applied, include/psdr/core/transform.h:91-94), m_scale, and the
   scene AABB the sampled directions are projected on (m_lower / m_upper, scene.cpp:135-141) */
#define PSDR_ENV_FROM_WORLD  0
#define PSDR_ENV_TO_WORLD    9
#define PSDR_ENV_SCALE      18
#define PSDR_ENV_LOWER      19
#define PSDR_ENV_UPPER      22

/* integrators (src/psdr.cpp:282-294; PathTracer is build-defined) */
#define PSDR_INTEGRATOR_DIRECT 0
#define PSDR_INTEGRATOR_PATH   1
#define PSDR_INTEGRATOR_FIELD  2
/* CollocatedIntegrator (build-defined, csrc/psdr_collocated.h): a point light of unit intensity at the camera position.  For a camera ray with origin o
   that hits `its`:  Li = f(its; wi = its.wi, wo = its.wi) / |its.p - o|^2  (0 on a miss), f = the BSDF value with its cosine, in the shading frame of the
   hit.  Emitters add nothing (no Le, no emitter sampling; a scene without any emitter is valid); no draws beyond the film jitter: two per camera slot,
   one per primary-edge slot.  Gradients: interior + primary edges -- a point seen from the camera is seen from the light, so there is no secondary-edge
   term and sppse is ignored.  The caller scales image, derivative images and adjoint image by the light's RGB intensity. */
#define PSDR_INTEGRATOR_COLLOCATED 3
/* PointLightIntegrator (build-defined, csrc/psdr_pointlight.h): a point light of unit intensity at the world position psdr_scene_set_point_light gave
   the handle.  For a camera ray that hits `its`, with dv = pL - its.p:  Li = f(its; wi = its.wi, wo = to_local(dv / |dv|)) * V(its.p, pL) / |dv|^2,
   V = 0 if the ray from its.p towards pL meets a surface at t in [RayEpsilon, |dv| - ShadowEpsilon).  Emitters add nothing; draws per slot: 2 (camera),
   1 (primary edge), 3 (shadow boundary, the first is used).  Gradients: interior + primary edges + the boundary of the moving shadow outline, which
   honours sppse and its shard range.  A render call of this kind without a light set is an error.  The caller scales by the light's RGB intensity. */
#define PSDR_INTEGRATOR_POINT 4
/* LightStageIntegrator (build-defined, csrc/psdr_lightstage.h): the L point lights psdr_scene_set_point_lights gave the handle, each of unit intensity,
   rendered from ONE camera hit per sample slot.  Plane l of every image is PSDR_INTEGRATOR_POINT's image under light l at the same options (same draws,
   same rng_offset for every light): psdr_render_c overwrites out_img [L][H*W*3]; psdr_render_d_fwd writes out_img [L][H*W*3] and out_dimg [K][L][H*W*3];
   psdr_render_d_rev reads adj_img [L][H*W*3] (and overwrites out_img [L][H*W*3] if given).  spp, sppe and sppse shard ranges are honoured as for kind 4.
   A render call of this kind without lights is an error.  The caller scales plane l by light l's RGB intensity. */
#define PSDR_INTEGRATOR_POINT_STACK 5
#define PSDR_POINT_LIGHTS_MAX 256
/* The light models of kinds 4 and 5 (psdr_scene_set_light / psdr_scene_set_lights).  PSDR_LIGHT_POINT: the text above.  PSDR_LIGHT_DISTANT: the light's
   vector is a DIRECTION d that points from the scene TOWARDS the light, of any non-zero length; with u = d / |d|
       Li = f(its; wi = its.wi, wo = to_local(u)) * V(its.p, u),   V = 0 if the ray (its.p, u) meets a surface at any t >= RayEpsilon.
   No 1 / r^2: the unit light gives unit IRRADIANCE to a surface that faces it (the caller scales by the irradiance, RGB), so a point light at c + R u
   with intensity R^2 tends to this model.  The gradient of the light is that of d as passed: it has no component along d and scales as 1 / |d|.
   The shadow-boundary term is that of the parallel projection along -u.  A distant light cannot reach a scene inside an environment map's bounding
   mesh: a render call of kind 4 or 5 with a distant light on such a scene is an error. */
#define PSDR_LIGHT_POINT   0
#define PSDR_LIGHT_DISTANT 1
/* FieldExtractionIntegrator fields (src/integrator/field.cpp:10-54) */
#define PSDR_FIELD_SILHOUETTE 0
#define PSDR_FIELD_POSITION   1
#define PSDR_FIELD_DEPTH      2
#define PSDR_FIELD_GEONORMAL  3
#define PSDR_FIELD_SHNORMAL   4
#define PSDR_FIELD_UV         5

/* Scene tables = everything Scene::configure() leaves on the device
   (reference src/scene/scene.cpp:56-278). */
typedef struct psdr_scene_desc {
    int32_t width, height;               /* RenderOption, types.h:171-182 */
    int32_t num_tris, num_meshes, num_bsdfs, num_emitters;
    int32_t num_sec_edges, num_prim_edges, num_texels, num_guide_cells;

    const float   *tri_info;             /* [T][PSDR_TRI_STRIDE]   scene.cpp:205-216; MUST be 16-byte aligned (rows are staged as float4) */
    const float   *tri_uv;               /* [T][PSDR_TRIUV_STRIDE] or NULL (all zero) */
    const int32_t *tri_mesh;             /* [T] */
    const int32_t *mesh_bsdf;            /* [M] bsdf id (Mesh::m_bsdf); -1 = the bounding mesh of the
                                            environment map (scene.cpp:135-172, bsdf == nullptr) */
    const int32_t *mesh_emitter;         /* [M] emitter id or -1 (Mesh::m_emitter) */
    const int32_t *bsdf_rec;             /* [Nb][PSDR_BSDF_STRIDE] */
    const float   *texels;               /* pool of Bitmap data; 3-ch textures interleaved RGB */
    const float   *emitter_f;            /* [Ne][PSDR_EMITTER_F_STRIDE] */
    const int32_t *emitter_i;            /* [Ne][PSDR_EMITTER_I_STRIDE] */
    const float   *face_cmf, *face_pmf;  /* per-emitter-mesh face distributions, mesh.cpp:248-249 */
    const float   *emitter_cmf, *emitter_pmf; /* [Ne] Scene::m_emitters_distrb, scene.cpp:183-196 */
    float          emitter_sum;
    const float   *cam;                  /* [PSDR_CAM_WORDS] */
    const float   *sec_edge;             /* [E][PSDR_SEDGE_STRIDE] scene.cpp:219-244 */
    const float   *sec_cmf, *sec_pmf;    /* [E] pmf = |e1| */
    float          sec_sum;
    const float   *prim_edge;            /* [Ep][PSDR_PEDGE_STRIDE] perspective.cpp:39-111 */
    const float   *prim_cmf, *prim_pmf;  /* [Ep] pmf = screen length */
    float          prim_sum;
    int32_t        guide_reso[3];        /* HyperCubeDistribution3f, src/core/cube_distrb.cpp */
    const float   *guide_cmf, *guide_pmf;/* [num_guide_cells] or NULL (no guiding) */
    float          guide_sum;
    /* EnvironmentMap (at most one, scene_loader.cpp:294-311): env_emitter = its index in the emitter
       tables or -1; its emitter_i row names the bounding mesh (scene.cpp:135-172).  The lat-long
       radiance bitmap lives in the texel pool (so d_texels / g_texels cover it). */
    int32_t        env_emitter;
    int32_t        env_tex[3];           /* texel offset, width, height of m_radiance */
    int32_t        env_reso[2];          /* m_cell_distrb resolution ((w-1)*2, (h-1)*2), envmap.cpp:14-15 */
    const float   *env_f;                /* [PSDR_ENV_WORDS] */
    const float   *env_cmf, *env_pmf;    /* [env_reso[0]*env_reso[1]] luminance*sin(theta), envmap.cpp:17-21 */
    float          env_sum;
    /* Bit t set = a BSDF of type t (PSDR_BSDF_*) occurs in bsdf_rec; 0 = unknown (the library then keeps
       the code of every BSDF type in its kernels).  A host that knows its materials sets it so that, e.g.,
       an all-diffuse scene runs the kernel variant compiled without the GGX / conductor-Fresnel code.
       Bits that are clear MUST be right: a cleared type is evaluated as diffuse.
       Bit PSDR_BSDF_MICROFACET (2) announces a MicrofacetBSDF record.  That type is never "unknown": with material_mask == 0 the caller
       promises that no PSDR_BSDF_MICROFACET record is present.  Bit PSDR_BSDF_MICROFACET_NORMAL (3) announces a normal-mapped one in the same way
       (never "unknown" either) and selects the same kernels as bit 2; bit PSDR_BSDF_MICROFACET_HEIGHT (4) does the same for a height-mapped one. */
    uint32_t       material_mask;
    /* [E][2] global triangle ids of the one or two faces adjacent to every secondary edge (second = -1 on a
       boundary edge), or NULL.  Not in the reference's SecondaryEdgeInfo (edge.h:27-65): the two rays that
       eval_secondary_edge (direct.cpp:246-254) starts ON the edge cannot hit these faces again in exact
       arithmetic (a line meets a plane once, at the edge point); in fp32 the rounded edge point lets a grazing
       ray re-hit them just above RayEpsilon -- ~3e-3 of the boundary term.  With the table the two rays skip
       the adjacent faces; without it they are traced as the reference does. */
    const int32_t *sec_edge_faces;
    /* [Ep][4] per primary edge: 1 / depth along the viewing direction (dot(vertex - camera, normalize(cam[PSDR_CAM_DIR])))
       of its two end points, then the global ids of its adjacent faces as int32 bit patterns (second = first on a boundary
       edge); or NULL.  When present the primary-edge term runs the reference's PSDR_PRIMARY_EDGE_VIS_CHECK variant
       (macros.h:13, integrator.cpp:105-108, perspective.cpp:91-96,171-196): an edge sample counts only if the edge point
       itself is visible from the camera (the ray through it with tmax = distance - 100 ShadowEpsilon hits nothing).  The
       reference keeps the sample-space z of the end points and unprojects the interpolated point; 1 / depth is affine along
       the film segment in the same way and distance = depth / cos is the same number in exact arithmetic, but
       sample-space z = far (1 - near / depth) / (far - near) holds only 3-4 digits of the depth in fp32 (near 0.1, depth
       500: +-0.15 units against the 1e-3 margin), and the edge's own faces -- met exactly AT the distance -- are skipped
       rather than left to round-off. */
    const float   *prim_edge_z;
} psdr_scene_desc;

/* psdr_render_opts.flags: execution strategy of the PathTracer interior term.
   default: the library chooses.  FUSED = one lane carries a whole path in registers.
   WAVEFRONT = one kernel per bounce over SoA path-state streams in HBM with wave-ballot stream
   compaction of the live paths between bounces (renderC and material-only renderD). */
#define PSDR_FLAG_FUSED     1
#define PSDR_FLAG_WAVEFRONT 2
/* Evaluate the three expressions the library replaces by fp32-robust equivalents in the reference's LITERAL
   form instead: the solid-angle hit point as p = ray(t) (scene.cpp:368), the rays that start on a secondary edge without skipping
   the adjacent faces (direct.cpp:246-254; as if sec_edge_faces were NULL), and "the camera sees p1" as the fp32 distance
   |its1.p - p1| < ShadowEpsilon (direct.cpp:262).  psdr_render_c / psdr_render_d_fwd only (reverse mode has no literal-form adjoint):
   makes the difference between the two forms measurable on the device against the oracle's reference_form. */
#define PSDR_FLAG_LITERAL_FORMS 4
/* psdr_render_c only: the caller is going to differentiate THIS render in reverse mode (renderD + enoki.backward: the primal image first, the adjoint image
   later).  Where the following psdr_render_d_rev would run a split launch whose value sweep is exactly this render -- PathTracer on a two-level scene, the
   traced wavefront, one chunk of slots -- the render runs with recording stages and the per-path records stay on the handle; a psdr_render_d_rev with the
   same options, the same tables (psdr_scene_set_tables with an identical descriptor in between is fine; the caller must not have overwritten them in
   place) and out_img = NULL then runs its adjoint kernel only (C4 shard: 15.6 of its 34.5 ms).  Where the wavefront does not apply (a scene without a
   tree: the 12-triangle cbox) the PathTracer render runs as the value kernel of a split reverse launch instead (image + one record per path) and a
   psdr_render_d_rev that asks for a geometry table (tri_info / cam_to_world) runs the adjoint kernel on it (cbox 512^2 x 64: 0.85 + 4.86 -> 1.25 + 4.0 ms).
   Ignored wherever neither applies (other integrators, paths deeper than 8, more slots than one chunk, option rev_split = 0). */
#define PSDR_FLAG_KEEP_RECORDS 8
/* psdr_render_d_fwd / psdr_render_d_rev with PSDR_INTEGRATOR_PATH: evaluate the secondary-edge boundary term of the PathTracer on the slots
   sppse / sppse_begin / sppse_end name (per slot a direct-source and an indirect-source boundary segment, each with a random
   walk of camera connections on the sensor side; max_depth = 1 is DirectIntegrator(1, 1)'s term draw for draw).  A slot of sampler 2 then
   consumes 11 max_depth - 9 draws (3 at max_depth = 1).  max_depth <= 8.  The descriptor's guiding grid guides the direct-source segment, psdr_scene_set_path_guide's the indirect-source segment (a guided
   slot warps its numbers, it draws no other ones).  Without the flag a PathTracer call
   ignores sppse, as it always did; other integrators ignore the flag.  Scene options pt_sedge (3: both segments, 1: direct source only,
   2: indirect source only, 0: neither) and pt_sedge_walk (0: the walk stops at its first vertex) are A/B switches for tests. */
#define PSDR_FLAG_PATH_SEDGES 16
#define PSDR_PATH_SEDGES_MAX_DEPTH 8

/* One render call = Integrator::renderC / renderD on one shard of the sample
   slots (src/integrator/integrator.cpp:13-119, src/integrator/direct.cpp). */
typedef struct psdr_render_opts {
    int32_t integrator;                  /* PSDR_INTEGRATOR_* */
    int32_t bsdf_samples, light_samples; /* DirectIntegrator ctor, direct.cpp:32-34 */
    int32_t max_depth;                   /* PathTracer; psdr_render_d_rev: up to 8 the per-lane path record lives in LDS, up to 250 in HBM */
    int32_t hide_emitters;               /* DirectIntegrator::m_hide_emitters */
    int32_t field;                       /* PSDR_FIELD_* */
    int32_t spp, sppe, sppse;            /* GLOBAL counts: normalisation + RNG stream index */
    int32_t spp_begin, spp_end;          /* this call evaluates s in [begin,end) of every pixel */
    int32_t sppe_begin, sppe_end;        /* slots [W*H*begin, W*H*end) of sampler 1 */
    int32_t sppse_begin, sppse_end;      /* slots [W*H*begin, W*H*end) of sampler 2 */
    int32_t flags;                       /* PSDR_FLAG_* (0 = library chooses) */
    uint64_t rng_offset[3];              /* draws already consumed per stream of sampler 0/1/2:
                                            the reference keeps the PCG32 states alive across
                                            render calls (scene.cpp:65-79) */
} psdr_render_opts;

/* Forward-mode tangent tables (d table / d P); any pointer may be NULL (= 0). */
typedef struct psdr_tangents {
    const float *d_tri_info;             /* [T][PSDR_TRI_STRIDE] */
    const float *d_texels;               /* [num_texels] */
    const float *d_emitter_rad;          /* [Ne][3] */
    const float *d_cam_to_world;         /* [16] row-major */
    const float *d_sec_edge;             /* [E][PSDR_SEDGE_STRIDE] (p0, e1 used... all 15) */
    const float *d_prim_edge;            /* [Ep][PSDR_PEDGE_STRIDE] (p0, p1 used) */
    const float *d_env_f;                /* [PSDR_ENV_WORDS] (from_world and scale used) */
} psdr_tangents;

/* Reverse-mode gradient tables (accumulated with +=); NULL = not wanted. */
typedef struct psdr_grads {
    float *g_tri_info;
    float *g_texels;
    float *g_emitter_rad;
    float *g_cam_to_world;
    float *g_sec_edge;
    float *g_prim_edge;
    float *g_env_f;
} psdr_grads;

typedef struct psdr_scene_s *psdr_scene_t;

/* error text of the last failing call on this thread */
const char *psdr_last_error(void);
/* "psdr-hip <version> gfx950" */
const char *psdr_version(void);
/* sizeof(psdr_scene_desc), sizeof(psdr_render_opts), sizeof(psdr_tangents), sizeof(psdr_grads):
   lets a foreign-language binding verify its struct mirrors before the first call */
int psdr_abi_struct_sizes(int32_t out[4]);

/* Scene handle; replaces Scene() / ~Scene() (src/scene/scene.cpp:19-41). */
int psdr_scene_create(psdr_scene_t *out);
int psdr_scene_destroy(psdr_scene_t h);
/* Developer options of a handle -- the A/B switches of tools and tests (the reference has none: its strategies are fixed by OptiX and
   Enoki); the library reads NO environment variable.  Names (value): bvh_refit, tiny_scene, two_level, wf_binned, wf_traced, sort_edges,
   tiny_variants, sink_private, aa_prims (0 / 1); bvh_build (1 device, 0 host, -1 by size); wide (0: never the 4-wide tree in the render kernels);
   rev_split, sedge_split (1 / 0 force, -1 default rule); pt_sedge (3 / 1 / 2 / 0) and pt_sedge_walk (0 / 1): see PSDR_FLAG_PATH_SEDGES; keep_records (0: PSDR_FLAG_KEEP_RECORDS is ignored); logd (0: PathTracer forward mode with tangents on
   diffuse albedo texels only runs the dual-number kernel, never the log-derivative one); rev_sorted (0: reverse PathTracer kernels
   scatter row adjoints on the spot); wf_geo (0: PathTracer geometry tangents through the fused kernel); tangent_live (0: no liveness mask); forest_min_inline (inline triangles a two-level tree needs at least: default 0 (6 = rooms only)); scratch_plain (1: scratch blocks of 64 MB and more come from hipMalloc instead of the stream-ordered pool -- process-wide, an experiment on TLB reach);
   own_pixels (0: the camera kernels always add to the image with atomics, also where one wave holds all samples of a pixel); emitter_pretest (0: BSDF-sampled rays whose hit matters only on an emitter -- DirectIntegrator, a PathTracer path's last vertex -- are traced without
   first meeting the emitters' primitives); occ_rows (0: the light rays of a scene without a tree test every kernel-argument primitive instead of
   the ones that can lie between the path vertex and the emitter sample); probe (0: no probe / trace / final launches);
   seed_cache (1 default: the fused PathTracer renderC launches on a scene without a tree load the seeded PCG32 state of
   their sample slots from a read-only table on the handle, filled once per (width * height, spp, spp range); 0: every kernel seeds its streams itself; same results
   either way); seed_cache_log2 (the largest launch that table serves, log2 of its slots at 16 bytes each: default 25 = 512 MB; larger launches seed themselves);
   logd_park (1 default: forward-mode PathTracer launches with ONE tangent set on albedo texels, on a plain diffuse scene without a tree, run the lean twin of the
   log-derivative kernel, which keeps a path's idle state in per-lane LDS columns instead of scratch memory -- where staged scene + columns fit six workgroups per CU
   and a forced lds_budget; 0: always the kernel without columns; same results either way);
   path_lean (1 default: fused PathTracer launches -- renderC, and forward mode with ONE tangent set on albedo texels -- on a plain diffuse scene without a tree run
   the lean twins where every wave of the launch sits on one pixel (64 samples per pixel in the call) and every primitive is an axis-aligned rectangle: material
   looked up once per vertex, film work on the scalar unit, slab-form ray tests only; 0: exactly the launches of before the twins; same results either way);
   trace_wg2 (dense trace kernel as two workgroups per CU: -1 by forest and launch size, 0 never, n > 0 always with stack columns of n entries);
   chunk_log2 (slots per chunk of the chunked launches, 0 = default); blocks_per_cu, camera_blocks, lds_budget, sink_rep, bvh_maxleaf (integers,
   0 = default where that makes sense); bvh_tcost (float).  Unknown names fail.  Options that change the tree take effect at the next psdr_bvh_build. */
int psdr_scene_set_option(psdr_scene_t h, const char *name, double value);

/* Replaces the table-publishing tail of Scene::configure (scene.cpp:199-244):
   remembers the caller-owned device tables. */
int psdr_scene_set_tables(psdr_scene_t h, const psdr_scene_desc *desc);

/* Replaces Scene_OptiX::configure + the OptiX GAS build
   (src/scene/scene_optix.cpp:34-72, include/psdr/scene/optix.h:277-340):
   builds the BVH over tri_info (p0,e1,e2) of the current tables.  When the triangle count is
   unchanged since the last build (an optimisation loop moving vertices) the tree is refitted on
   the device instead of rebuilt (OptiX's build is a device build too); it is rebuilt when the
   refitted boxes have grown by 30 % in area or after 64 refits.  psdr_scene_set_option(h, "bvh_refit", 0)
   forces a rebuild every time (the library reads no environment variable). */
int psdr_bvh_build(psdr_scene_t h, void *stream);
/* out = { full builds, refits, inner nodes, tree depth } of this handle (diagnostics) */
int psdr_bvh_stats(psdr_scene_t h, int32_t out[4]);
/* out = { primitives carried in the kernel arguments (triangles or parallelograms), trees of a two-level scene,
   inline triangles of a two-level scene, leaf triangles in the tree(s), 1 if the tree was built on the device,
   how many of [0] are axis-aligned rectangles in slab form, 1 if the light rays of a scene without a tree test occluder rows only, the most rows any of
   those entries names } -- what psdr_bvh_build chose for the current tables (diagnostics; bench.py prices its
   per-ray arithmetic floor from [0]).  No reference counterpart: OptiX hides its acceleration structure. */
int psdr_scene_info(psdr_scene_t h, int32_t out[8]);

/* Replaces Scene_OptiX::ray_intersect + the OptiX programs
   (scene_optix.cpp:81-126, cuda/psdr_cuda.cu:9-45): closest hit with
   t in [1e-3, tmax] for m rays given as 7 SoA streams; writes mesh id,
   GLOBAL triangle id (-1 on miss) and the barycentrics of vertex 1 and 2. */
int psdr_trace(psdr_scene_t h, int32_t m,
               const float *ox, const float *oy, const float *oz,
               const float *dx, const float *dy, const float *dz,
               const float *tmax,
               int32_t *out_shape, int32_t *out_tri, float *out_u, float *out_v,
               void *stream);

/* Replaces Integrator::renderC (integrator.cpp:13-29): out_img [H*W*3],
   overwritten with (1/spp) * sum over this shard's slots. */
int psdr_render_c(psdr_scene_t h, const psdr_render_opts *opts,
                  float *out_img, void *stream);

/* Replaces Integrator::renderD followed by enoki forward(P)
   (integrator.cpp:32-60, examples/run_test.py:126-129): interior +
   primary-edge + secondary-edge terms; out_dimg [K][H*W*3]. */
int psdr_render_d_fwd(psdr_scene_t h, const psdr_render_opts *opts,
                      int32_t K, const psdr_tangents *tangents,
                      float *out_img, float *out_dimg, void *stream);

/* Replaces Integrator::renderD followed by enoki backward(loss)
   (docs/inverse_diff_render.rst): adj_img [H*W*3] = dLoss/dImage; gradients
   are scatter-added into `grads`. out_img may be NULL. */
int psdr_render_d_rev(psdr_scene_t h, const psdr_render_opts *opts,
                      const float *adj_img, float *out_img,
                      const psdr_grads *grads, void *stream);

/* Replaces DirectIntegrator::preprocess_secondary_edges (direct.cpp:166-204):
   out_mass [reso0*reso1*reso2] = mean over nrounds of per-cell max-RGB. */
int psdr_guide_build(psdr_scene_t h, const psdr_render_opts *opts,
                     const int32_t reso[4], int32_t nrounds,
                     float *out_mass, void *stream);

/* Guiding grids of the PathTracer's secondary-edge term (PSDR_FLAG_PATH_SEDGES; no reference counterpart: the
   snapshot has no PathTracer).  A slot evaluates two boundary segments; each may have a 3-D grid with the semantics
   of HyperCubeDistribution3f over the three numbers that decide it: segment A (direct source) over the slot's
   sample3 -- the descriptor's guide_* grid, the very cube of DirectIntegrator's term -- and segment B (indirect
   source) over (sample3[0], the two sphere-direction numbers).

   psdr_scene_set_path_guide installs segment B's grid on the handle: reso [3], cmf / pmf [reso0*reso1*reso2] and
   sum as psdr_cube_sample_reuse takes them; the device tables stay the caller's.  cmf == NULL clears the grid.
   psdr_scene_set_tables drops it (as it replaces every other table): set it again after every set_tables.

   psdr_path_guide_build estimates a grid's mass for segment 1 (A) or 2 (B), unguided (any grid that is set is
   ignored), with opts->max_depth and the handle's pt_sedge_walk:
   out_mass [reso0*reso1*reso2] = mean over nrounds of the sum over the cell's reso[3] streams of
   hmax(sum over the segment's camera connections of |value|) / reso[3].  At max_depth 1 the mass of segment 1 is
   psdr_guide_build's. */
int psdr_scene_set_path_guide(psdr_scene_t h, const int32_t reso[3], const float *cmf, const float *pmf, float sum);
/* The light of PSDR_INTEGRATOR_POINT.  pos: world position (host, copied).  d_pos: HOST array [K][3] of position tangents (copied; K = 0..3) or NULL --
   psdr_render_d_fwd reads the first K' rows of its own K, missing rows are zero.  g_pos: DEVICE array [3] that psdr_render_d_rev adds the gradient of
   the position into (+=; the caller zeroes it and keeps it alive), or NULL.  pos == NULL removes the light.  The light survives psdr_scene_set_tables. */
int psdr_scene_set_point_light(psdr_scene_t h, const float pos[3], int32_t K, const float *d_pos, float *g_pos);
/* The lights of PSDR_INTEGRATOR_POINT_STACK, L = 1 .. PSDR_POINT_LIGHTS_MAX.  pos: HOST array [L][3] of world positions (copied).  d_pos: HOST array
   [K][L][3] of position tangents (copied; K = 0..3) or NULL -- psdr_render_d_fwd reads the first K' sets of its own K, missing sets are zero.  g_pos: DEVICE
   array [L][3] that psdr_render_d_rev adds the gradients of the positions into (+=; the caller zeroes it and keeps it alive), or NULL.  pos == NULL or
   L == 0 removes the lights.  They survive psdr_scene_set_tables and are independent of psdr_scene_set_point_light: PSDR_INTEGRATOR_POINT keeps reading
   its own light. */
int psdr_scene_set_point_lights(psdr_scene_t h, int32_t L, const float *pos, int32_t K, const float *d_pos, float *g_pos);
/* The same two with a light model per light (PSDR_LIGHT_POINT / PSDR_LIGHT_DISTANT); the two above mean PSDR_LIGHT_POINT.  v: the position, or the
   direction TOWARDS the light (any non-zero, finite length); d_v: its tangents; g_v: the gradient of that vector as passed -- for a direction it is
   tangential (no component along d) and scales as 1 / |d|.  kinds: HOST array [L] (copied); a stack may mix the kinds in any order.  Errors: an unknown
   kind, a vector that is not finite, a direction that is all zero.  v == NULL (or L == 0) removes the light(s). */
int psdr_scene_set_light(psdr_scene_t h, int32_t kind, const float v[3], int32_t K, const float *d_v, float *g_v);
int psdr_scene_set_lights(psdr_scene_t h, int32_t L, const int32_t *kinds, const float *v, int32_t K, const float *d_v, float *g_v);
int psdr_path_guide_build(psdr_scene_t h, const psdr_render_opts *opts, int32_t segment,
                          const int32_t reso[4], int32_t nrounds,
                          float *out_mass, void *stream);

/* Replaces HyperCubeDistribution<ndim>::sample_reuse (src/core/cube_distrb.cpp:41-48), ndim = 2 or 3:
   samples [m][ndim] are warped IN PLACE, out_pdf [m] = pmf * n.  cmf / pmf / sum as DiscreteDistribution
   holds them (src/core/pmf.cpp:7-14: inclusive prefix sum, unnormalised), reso [ndim], n = prod(reso).
   A one-cell grid leaves the samples as they are with pdf 1, whatever its mass (DiscreteDistribution's
   size-1 shortcut); on more cells an all-zero mass (sum = 0) gives pdf 0 (the reference: 0 / 0). */
int psdr_cube_sample_reuse(int32_t ndim, const int32_t *reso, const float *cmf, const float *pmf, float sum,
                           int32_t n, int32_t m, float *samples, float *out_pdf, void *stream);
/* Replaces Scene::sample_boundary_segment_direct (src/scene/scene.cpp:456-492) over the tables of a
   scene descriptor -- the one psdr_scene_set_tables takes; no handle, no tree: sample3 [m][3], active [m]
   (NULL = all).  out_p0, out_edge_dir, out_edge2, out_p2, out_n [m][3]; out_pdf [m] (0 where invalid),
   out_valid [m]; out_edge [m] = the secondary-edge row drawn, out_s1 [m] = the sample reused along it.
   Every emitter kind is sampled as the render kernels do (scene.cpp:427-447). */
int psdr_sample_boundary_segment_direct(const psdr_scene_desc *desc, int32_t m, const float *sample3,
                                        const uint8_t *active, float *out_p0, float *out_edge_dir,
                                        float *out_edge2, float *out_p2, float *out_n, float *out_pdf,
                                        uint8_t *out_valid, int32_t *out_edge, float *out_s1, void *stream);

/* ---- the differentiable table chain of Scene::configure as kernels (csrc/psdr_tables.hip) -------------------------------------
   All pointers are device pointers; vertices [V][3], faces [T][3] int32 (global vertex ids), rows [T][row_stride >= 22] in the
   TriangleInfo layout (PSDR_TRI_STRIDE words when written straight into tri_info), edges [E][5] int32 = v0, v1, face0, face1
   (-1: boundary), opposite vertex of face0 (global ids; Mesh::m_edge_indices, mesh.cpp:154-196).  The *_rev entry points ADD the
   adjoints into a_v / a_rows / a_w2s (the caller zeroes them).  The *_jvp entry points are forward mode: they take the primal inputs and
   ONE tangent per differentiable input (a null tangent = zero) and WRITE the tangent of the differentiable output, with the launches and
   layouts of the primal entry.  The keep masks are primal-only: no tangent flows through them. */
/* World positions (Mesh::configure, src/shape/mesh.cpp:226-232: transform_pos of include/psdr/core/transform.h:84-88 by the mesh's to_world):
   v_raw [V][3] object-space positions, vmesh [V] int32 = the mesh of every vertex, mats [M][16] row-major to_world matrices.
   The reverse entry point WRITES a_raw (adjoint of v_raw; the matrices carry no gradient on this path: the caller keeps the torch chain when they do). */
int psdr_geo_world_vertices_fwd(int32_t V, const float *v_raw, const int32_t *vmesh, const float *mats, float *v_world, void *stream);
int psdr_geo_world_vertices_rev(int32_t V, const float *v_raw, const int32_t *vmesh, const float *mats, const float *v_world, const float *a_world, float *a_raw,
                                void *stream);
/* t_world [V][3] from t_raw [V][3] and t_mats [M][16] (either may be null); v_world = the output of the forward entry. */
int psdr_geo_world_vertices_jvp(int32_t V, const float *v_raw, const int32_t *vmesh, const float *mats, const float *v_world, const float *t_raw, const float *t_mats,
                                float *t_world, void *stream);
/* process_mesh (src/shape/mesh.cpp:20-51): rows = p0 e1 e2 n0 n1 n2 face_normal face_area with area-weighted vertex normals;
   vsum [V][3] = scratch kept for the adjoint (the un-normalised vertex normals). */
int psdr_geo_tri_rows_fwd(int32_t V, int32_t T, const float *v, const int32_t *faces, float *vsum, float *rows, int32_t row_stride, void *stream);
int psdr_geo_tri_rows_rev(int32_t V, int32_t T, const float *v, const int32_t *faces, const float *vsum, const float *a_rows, int32_t row_stride,
                          float *a_vsum /* scratch [V][3] */, float *a_v, void *stream);
/* t_rows [T][row_stride] from t_v [V][3] (vsum: as the forward entry left it); the tangents of the vertex-normal sums are accumulated in
   double like the sums themselves.  A degenerate face has zero face-normal and area tangents. */
int psdr_geo_tri_rows_jvp(int32_t V, int32_t T, const float *v, const int32_t *faces, const float *vsum, const float *t_v, int32_t row_stride,
                          float *t_vsum /* scratch [V][3] */, float *t_rows, void *stream);
/* SecondaryEdgeInfo of EVERY candidate edge (Mesh::configure, mesh.cpp:251-270): info [E][16] = p0 e1 n0 n1 p2 is_boundary, and
   keep [E] = 1 where the coplanar filter of scene.cpp:219-244 keeps the edge (the caller compacts). */
int psdr_geo_sec_edges_fwd(int32_t E, const int32_t *edges, const float *v, const float *rows, int32_t row_stride, float *info, uint8_t *keep, void *stream);
int psdr_geo_sec_edges_rev(int32_t E, const int32_t *edges, const float *a_info, float *a_v, float *a_rows, int32_t row_stride, void *stream);
/* t_info [E][16] from t_v [V][3] and t_rows [T][row_stride] (either may be null); a boundary edge's n1 tangent is zero. */
int psdr_geo_sec_edges_jvp(int32_t E, const int32_t *edges, const float *t_v, const float *t_rows, int32_t row_stride, float *t_info, void *stream);
/* PrimaryEdgeInfo of every candidate edge for one sensor (PerspectiveCamera::configure, src/sensor/perspective.cpp:39-111):
   cam22 = world_to_sample (16, row-major), camera position (3), viewing direction (3); face_normals [E] = 1 where the edge's mesh uses
   face normals; rows8 [E][PSDR_PEDGE_STRIDE], z4 [E][4] (psdr_scene_desc::prim_edge_z), keep [E] = the silhouette test. */
int psdr_geo_prim_edges_fwd(int32_t E, const int32_t *edges, const uint8_t *face_normals, const float *v, const float *rows, int32_t row_stride,
                            const float *cam22, float *rows8, float *z4, uint8_t *keep, void *stream);
int psdr_geo_prim_edges_rev(int32_t E, const int32_t *edges, const float *v, const float *cam22, const float *a_rows8, float *a_v, float *a_w2s /* [16] */,
                            void *stream);
/* t_rows8 [E][PSDR_PEDGE_STRIDE] from t_v [V][3] and t_w2s [16] (either may be null): the film positions' tangents; edge normal and length
   come from detached end points (perspective.cpp) and get zero.  The rows enter only the silhouette test, so they take no tangent. */
int psdr_geo_prim_edges_jvp(int32_t E, const int32_t *edges, const float *v, const float *cam22, const float *t_v, const float *t_w2s /* [16] */, float *t_rows8,
                            void *stream);

/* The kept edges of a candidate table as a table of the SAME capacity, with the count left on the device (scene.cpp:219-244 and
   perspective.cpp:96-111 compress the kept edges and build a DiscreteDistribution over their lengths, pmf.cpp:7-21, inside one Enoki trace;
   an eager host chain would read the number of kept edges back to size the result).  rows [E][S], keep [E]; the weight of a row is its
   word w0 (wn = 1) or the norm of words w0..w0+2 (wn = 3).  aux [E][aux_stride] 32-bit words of which the first A travel with the row
   (A = 0: none).  Outputs: rows_out [E][S] / aux_out [E][A] = the kept rows in their order, zero behind them; pos [E] = the new row of
   edge e or -1; pmf / cmf [E] = weight / sum and its running sum (cmf = 1 from the last kept row on, so a lower-bound search for u < 1
   never leaves the kept rows; the host passes sum = 1); header [2] = {number of kept rows as int bits, sum of the weights}.
   scratch: 4 * ceil(E / 1024) words.  _rev WRITES a_rows [E][S] (the adjoint of rows) from a_rows_out; _jvp WRITES t_rows_out [E][S]
   (row pos[e] = t_rows row e, every other row zero). */
int psdr_geo_compact_edges_fwd(int32_t E, const float *rows, int32_t S, const uint8_t *keep, int32_t w0, int32_t wn, const void *aux, int32_t aux_stride, int32_t A,
                               void *scratch, float *rows_out, void *aux_out, int32_t *pos, float *pmf, float *cmf, float *header, void *stream);
int psdr_geo_compact_edges_rev(int32_t E, int32_t S, const int32_t *pos, const float *a_rows_out, float *a_rows, void *stream);
int psdr_geo_compact_edges_jvp(int32_t E, int32_t S, const int32_t *pos, const float *t_rows, float *t_rows_out, void *stream);
/* Mesh areas and the emitter tables (scene.cpp:183-196, area.cpp:10-16, mesh.cpp:244-249) without a host round trip: face_offset [M + 1],
   mesh_emitter [M] (-1: none), emitter_i [Ne][PSDR_EMITTER_I_STRIDE], radiance [Ne][3], env_weight [Ne] (< 0: an area light; otherwise the
   sampling weight of the environment map).  Outputs: mesh_area [M]; emitter_f [Ne][PSDR_EMITTER_F_STRIDE]; emitter_pmf / emitter_cmf [Ne]
   NORMALISED (the host passes emitter_sum = 1); face_pmf / face_cmf = the face-area distributions of the area lights' meshes at
   emitter_i[.][3] (unnormalised, their sums in emitter_f[.][5]). */
int psdr_geo_emitter_tables(int32_t M, const float *rows, int32_t row_stride, const int32_t *face_offset, const int32_t *mesh_emitter, int32_t Ne, const int32_t *emitter_i,
                            const float *radiance, const float *env_weight, float *mesh_area, float *emitter_f, float *emitter_pmf, float *emitter_cmf, float *face_pmf,
                            float *face_cmf, void *stream);

/* ---- LargeSteps: u = (I + lambda L) x and x = (I + lambda L)^-1 b on vertex tables (csrc/psdr_smooth.hip) ----------------------
   The parameterisation of "Large Steps in Inverse Rendering" (Nicolet, Jacobson, Jakob 2021) for per-vertex shape optimisation; the
   reference has no counterpart.  L is the combinatorial Laplacian of the mesh's unique undirected edges: an edge shared by any number
   of faces or repeated by a duplicated face counts once, an edge (a, a) of a degenerate face is dropped, a vertex no face uses has the
   identity row.  Tables are [V][3] float, device, caller-owned.  The solve is conjugate gradients on the three columns in lockstep
   (csrc/psdr_smooth.h): it stops when every column has ||r|| <= tol ||b|| or at max_iter; a column with ||b|| = 0 returns exact zeros.
   A solve that does not converge is NOT an error (psdr_smooth_info reports it); non-finite input gives non-finite output after at most
   max_iter iterations.  Two launch forms, chosen by the option "one_workgroup": 1 = the whole solve in one launch of one workgroup
   (at most one_workgroup_limit vertices, else an error), 0 = two launches per iteration with every scalar on the device, -1 (default) =
   by the vertex count.  Either form is enqueued on the caller's stream and never waits on the host; psdr_smooth_info is the one call
   that waits.  The handle owns the adjacency and the work vectors: solves on one handle run one behind the other. */
typedef struct psdr_smooth_s *psdr_smooth_t;
typedef struct psdr_smooth_info_s {
    int32_t iterations;             /* CG steps of the handle's last solve */
    int32_t converged;              /* 1: every column met the tolerance */
    int32_t form;                   /* 1 one workgroup, 0 multi launch, -1 no solve yet */
    int32_t launches;               /* kernel launches the last solve enqueued */
    float rel_residual[3];          /* ||r|| / ||b|| per column (of the recurrence; 0 for a zero column) */
    int32_t one_workgroup_limit;    /* most vertices the one-workgroup form holds */
    int32_t one_workgroup_default;  /* option -1: meshes up to this many vertices take it */
    int32_t num_vertices;
    int32_t num_entries;            /* directed entries of the adjacency = 2 x unique edges */
    int32_t long_rows;              /* rows gathered by a whole wave (more than 64 neighbours) */
} psdr_smooth_info_t;
/* faces: HOST [F][3] int32; an index outside [0, V) is an error.  Builds and uploads the adjacency (CSR, rows sorted by column). */
int psdr_smooth_create(int32_t V, int32_t F, const int32_t *faces, psdr_smooth_t *out);
void psdr_smooth_destroy(psdr_smooth_t h);
int psdr_smooth_set_option(psdr_smooth_t h, const char *name, int value);
/* u = (I + lambda L) x; lambda >= 0; x and u must not alias. */
int psdr_smooth_apply(psdr_smooth_t h, float lambda, const float *x, float *u, void *stream);
/* x = (I + lambda L)^-1 b; x0 = the initial guess or NULL (zero); x0 may be x, b may not.  tol > 0, max_iter >= 1. */
int psdr_smooth_solve(psdr_smooth_t h, float lambda, const float *b, const float *x0, float *x, float tol, int32_t max_iter, void *stream);
/* Waits for the handle's last solve. */
int psdr_smooth_info(psdr_smooth_t h, psdr_smooth_info_t *out);

/* Gradient layout of the last psdr_render_d_rev on this handle (diagnostics: which destination each adjoint of the camera
   term went to; zeros before the first call).  out = {
     [0] texel words cached in LDS (0: global atomics), [1] emitter-radiance words cached, [2] environment-map words cached,
     [3] triangle rows cached (the rest go through global atomics), [4] copies of the LDS cache,
     [5] lane-private emitter rows, [6] 1 if those live in registers, [7] deferred row columns per lane,
     [8] camera launch: -1 none, 0 one kernel, 1 value + adjoint kernel, 2 the same with the wavefront value sweep, 3 adjoint kernel
         on kept records, 4 probe pass + reverse kernel,
     [9] copies of the primary-edge table (0: no primary-edge launch), [10] 1 if cached rows are addressed by triangle (slot = triangle),
     [11] 1 if the path records live in HBM, [12] [13] cache slots of the private rows, [14] hot rows the tree build chose,
     [15] 1 if the primary-edge slots ran sorted by pixel } */
int psdr_scene_rev_layout(psdr_scene_t h, int32_t out[16]);

/* Seed table of the handle (option seed_cache; diagnostics): out = { [0] slots the table holds seeds for (0: none), [1] bytes allocated,
   [2] fills since the handle was created (one per change of width * height, spp or spp range), [3] camera launches served from the table }. */
int psdr_scene_seed_info(psdr_scene_t h, int64_t out[4]);

/* Log-derivative camera launches of the handle (options logd, logd_park; diagnostics): out = { [0] launches since the handle was created, [1] those the lean
   twin ran, [2] those of the lean twin that loaded their seeds from the seed table, [3] dynamic LDS bytes per workgroup of the last lean launch (staged
   scene + parking columns; 0: none yet) }. */
int psdr_scene_logd_info(psdr_scene_t h, int64_t out[4]);

/* Fused PathTracer camera launches of the handle on flag set 8, plain diffuse without a tree (option path_lean; diagnostics): out = { [0] renderC launches the lean
   twin ran, [1] K = 1 log-derivative launches the lean twin ran (counted by psdr_scene_logd_info as lean launches too), [2] renderC launches and [3] K = 1
   log-derivative launches the selection rule left to the other kernels }. */
int psdr_scene_path_lean_info(psdr_scene_t h, int64_t out[4]);

/* Counters of the last render call on this handle (host values):
   [0] rays traced, [1] camera slots, [2] primary-edge slots, [3] secondary-edge slots. */
int psdr_get_counters(psdr_scene_t h, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PSDR_HIP_H */
