/* lrhost.h — C ABI of the host-side scene library (liblrhost.so): parse a LuisaRender scene
 * description, flatten it into the POD tables of lr_scene.h, build the wide BVH, write images.
 *
 * Stands in for the reference's host build phase, which is C++ against LuisaCompute headers
 * that are absent from the snapshot:
 *   SceneParser::parse      src/sdl/scene_parser.cpp:401-407
 *   Scene::create           src/base/scene.cpp:201-233
 *   Pipeline::create        src/base/pipeline.cpp:44-99   (registries, uploads)
 *   Geometry::build         src/base/geometry.cpp:12-163
 *   save_image              src/util/imageio.cpp:694-726
 * Conventions: 0 = OK, negative = error (message via lrhost_last_error, thread-local);
 * nothing throws or aborts across this boundary.
 */
#ifndef LRHOST_H
#define LRHOST_H

#include "lr_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrhost_scene lrhost_scene;

#define LRHOST_OK 0
#define LRHOST_ERROR (-1)

/* `-D key=value` command-line macros (src/apps/cli.cpp:105-152) are passed as parallel arrays */
int lrhost_scene_load_file(const char *path, const char *const *macro_keys, const char *const *macro_values,
                           int macro_count, lrhost_scene **out);
int lrhost_scene_load_string(const char *source, const char *virtual_path, int is_json,
                             const char *const *macro_keys, const char *const *macro_values,
                             int macro_count, lrhost_scene **out);
/* bake instances + build the 4-wide BVH consumed by lrhip_upload_scene */
int lrhost_scene_build_accel(lrhost_scene *scene);
/* Motion blur.  The reference renders a frame as a sequence of shutter samples (Camera::shutter_samples,
 * src/base/camera.cpp:163-203): for each one the scene is moved to the sample's time (Pipeline::update pipeline.cpp:101-113,
 * Geometry::update geometry.cpp:194-216) and `spp` samples per pixel are rendered with their radiance scaled by `weight`
 * (src/base/integrator.cpp:91-95).  A static camera has ONE sample (shutter_span.x, 1, spp).
 *   lrhost_scene_set_time: re-evaluates every animated transform (src/transforms/lerp.cpp; instances, cameras, environment)
 *   and refits the BVH when it is built; the tables behind lrhost_scene_view change in place (*updated = whether anything
 *   moved: upload the scene again then). */
int lrhost_scene_set_time(lrhost_scene *scene, float time, int *updated);
/* Moving instances by matrices the caller holds (Geometry::update, geometry.cpp:194-216; the host mirror of lrhip.h's
 * lrhip_set_instance_transforms): object_to_world[i] -- float[16], column-major, the layout of lr_instance.object_to_world -- becomes the
 * matrix of instance instances[i], or of instance i when `instances` is NULL (then count <= instance_count).  The baked triangles of
 * these instances are re-baked and the BVH is refitted over the same topology when it is built; the tables behind lrhost_scene_view
 * change in place (upload the scene again, or lrhip_update_scene).  An error, with nothing changed, for an id out of range or listed
 * twice, a non-finite matrix element, or NULL matrices with count > 0.  A later lrhost_scene_set_time moves the instances that carry
 * an animated transform to their transform's value again; the others keep what this call gave them.                              */
int lrhost_scene_set_instance_transforms(lrhost_scene *scene, uint64_t count, const uint32_t *instances, const float *object_to_world);
/* Deforming a mesh (the host mirror of lrhip.h's lrhip_set_mesh_vertices, which has the semantics): vertices [first_vertex, first_vertex + count)
 * of mesh `mesh` get positions[i] (float[3], packed, object space) and, when `normals` is not NULL, normals[i]; u v stay.  flags: 0 or
 * LRHIP_MESH_RECOMPUTE_NORMALS (normals must be NULL then), which recomputes the normals of all vertices of the mesh by lrhip.h's
 * definition, as a plain sequential loop.  The baked triangles of every instance of the mesh are re-baked and the BVH is refitted over the
 * same topology when it is built; the tables behind lrhost_scene_view change in place (lrhip_update_scene, or upload the scene again).
 * An error, with nothing changed, for a mesh or a range out of bounds, a non-finite element, NULL positions with count > 0, normals
 * together with the flag, unknown flags, and for a mesh of which an instance carries a light: tri_alias and tri_pdf are not rebuilt.
 * A later lrhost_scene_set_time re-bakes animated instances from the new vertices.                                                      */
int lrhost_scene_set_mesh_vertices(lrhost_scene *scene, uint32_t mesh, uint32_t first_vertex, uint64_t count, const float *positions,
                                   const float *normals, uint32_t flags);
int lrhost_scene_shutter_sample_count(const lrhost_scene *scene, int camera_index);
int lrhost_scene_shutter_sample(const lrhost_scene *scene, int camera_index, int sample_index, float *time, float *weight, uint32_t *spp);
int lrhost_scene_camera_count(const lrhost_scene *scene);
/* fill *out with pointers into `scene` (valid until lrhost_scene_destroy) */
int lrhost_scene_view(const lrhost_scene *scene, int camera_index, lr_scene *out);
const char *lrhost_scene_camera_file(const lrhost_scene *scene, int camera_index);
int lrhost_scene_has_lighting(const lrhost_scene *scene);
/* The AOV integrator (lr_integrator.kind == LR_INTEGRATOR_AOV, components in lr_integrator.flags; src/integrators/aov.cpp:48-87):
 * noisy_count (samples per pixel, in place of the camera's spp; at least 8) and the dump strategy (LR_AOV_DUMP_*).  An error for
 * any other integrator. */
int lrhost_scene_aov_settings(const lrhost_scene *scene, uint32_t *noisy_count, uint32_t *dump);
/* The AOV integrator's denoise properties (ours; the reference ignores properties it does not know): denoise { false },
 * denoise_iterations, denoise_sigma_color / _normal / _depth and denoise_demodulate, with lrhip.h's LRHIP_DENOISE_DEFAULT_* where the
 * scene sets none.  sigmas = { color, normal, depth }.  `denoise { true }` needs the components sample, albedo, normal and depth: a
 * scene that switches one of them off fails to load.  An error for any other integrator. */
int lrhost_scene_aov_denoise(const lrhost_scene *scene, uint32_t *enabled, uint32_t *iterations, uint32_t *demodulate, float sigmas[3]);
void lrhost_scene_destroy(lrhost_scene *scene);

int lrhost_save_image(const char *path, const float *rgba, uint32_t width, uint32_t height);
/* the same for 1 (HDR: gray; EXR: one channel named "A"), 3 (RGB) or 4 interleaved float channels per pixel */
int lrhost_save_image_channels(const char *path, const float *pixels, uint32_t width, uint32_t height, uint32_t channels);
/* load to float RGBA (row 0 = top); caller frees with lrhost_free */
int lrhost_load_image(const char *path, float **rgba, uint32_t *width, uint32_t *height, uint32_t *channels);
void lrhost_free(void *p);

/* sizeof() of the lr_scene.h structs by name ("lr_scene", "lr_surface", ...) and of lrhip.h's lrhip_denoise_params, for FFI layout checks */
uint64_t lrhost_sizeof(const char *struct_name);

void lrhost_set_log_level(int level); /* 0 silent, 1 warnings, 2 info */
const char *lrhost_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LRHOST_H */
