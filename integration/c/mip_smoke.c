/* A plain C99 host for libmi_instance_pipeline.so: what the reference-side shim does, minus Rust
 * ("exercised only through a C test driver"). Builds a tiny scene, runs one frame
 * with host output pointers and prints the draw count and a checksum of the command bytes.
 *   gcc -std=c99 -I include integration/c/mip_smoke.c -L renderer_amd/lib -lmi_instance_pipeline -o mip_smoke */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_instance_pipeline.h"

int main(void) {
  enum { N = 1000 };
  MipConfig cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg;
  cfg.max_instances = N;
  cfg.max_meshes = 1;
  MipContext* ctx = NULL;
  int32_t rc = mip_create(&cfg, &ctx);
  if (rc != MIP_OK) {
    printf("mip_create: %d\n", rc);
    return 10 - rc;
  }
  MipMesh mesh;
  memset(&mesh, 0, sizeof mesh);
  for (int a = 0; a < 3; ++a) {
    mesh.aabb_min[a] = -0.5f;
    mesh.aabb_max[a] = 0.5f;
  }
  mesh.n_lods = 2;
  mesh.index_len[0] = 36;
  mesh.index_len[1] = 18;
  mesh.index_offset[1] = 36;
  static float pos[N * 3], rot[N * 4], scale[N];
  static uint32_t mesh_id[N];
  for (int i = 0; i < N; ++i) { /* a 10 x 10 x 10 lattice in front of the default camera */
    pos[3 * i + 0] = (float)(i % 10) * 3.0f - 13.5f;
    pos[3 * i + 1] = (float)((i / 10) % 10) * 3.0f - 13.5f;
    pos[3 * i + 2] = (float)(i / 100) * 6.0f + 4.0f;
    rot[4 * i + 3] = 1.0f;
    scale[i] = 1.0f;
  }
  if ((rc = mip_set_mesh_table(ctx, &mesh, 1)) || (rc = mip_set_instances(ctx, pos, rot, scale, mesh_id, N))) {
    printf("setup: %d %s\n", rc, mip_last_error(ctx));
    return 10 - rc;
  }
  /* the reference's default camera: eye (0,1,2), looking down +z, fov 70 deg, aspect 2, near 0.1, far 100;
   * planes as -(row3 +- row k) of projection * view, order L R B T N F (src/ecs.rs:78-90) */
  MipFrame frame;
  memset(&frame, 0, sizeof frame);
  const float t = 0.70020754f /* tan(35 deg) */, aspect = 2.0f, n = 0.1f, f = 100.0f;
  const float px = 1.0f / (aspect * t), py = 1.0f / t, pz = f / (f - n), pw = -(f * n) / (f - n);
  const float eye[3] = {0.0f, 1.0f, 2.0f};
  /* rows of projection * view with view = translate(-eye) */
  const float r0[4] = {px, 0, 0, -px * eye[0]}, r1[4] = {0, py, 0, -py * eye[1]}, r2[4] = {0, 0, pz, -pz * eye[2] + pw},
              r3[4] = {0, 0, 1, -eye[2]};
  const float* rows[3] = {r0, r1, r2};
  for (int k = 0; k < 3; ++k)
    for (int c = 0; c < 4; ++c) {
      frame.planes[(2 * k) * 4 + c] = -(r3[c] + rows[k][c]);
      frame.planes[(2 * k + 1) * 4 + c] = -(r3[c] - rows[k][c]);
    }
  memcpy(frame.cam_pos, eye, sizeof eye);
  static float model[N * 16];
  static uint32_t bitmap[(N + 31) / 32];
  static MipDrawIndexedIndirectCommand cmds[N];
  uint32_t count = 0, index_total = 0;
  MipOutputs out;
  memset(&out, 0, sizeof out);
  out.model = model;
  out.visible_bitmap = bitmap;
  out.draw_cmds = cmds;
  out.draw_count = &count;
  out.draw_index_total = &index_total;
  out.flags = MIP_OUT_HOST;
  if ((rc = mip_run(ctx, &frame, &out))) {
    printf("mip_run: %d %s\n", rc, mip_last_error(ctx));
    return 10 - rc;
  }
  uint32_t visible = 0, sum = 0;
  for (uint32_t w = 0; w < (N + 31) / 32; ++w)
    for (uint32_t b = bitmap[w]; b; b &= b - 1) ++visible;
  for (uint32_t k = 0; k < count; ++k) sum = sum * 31u + cmds[k].indexCount + cmds[k].firstIndex * 7u + cmds[k].firstInstance * 13u;
  /* the running firstIndex must be the sum of the earlier index counts */
  uint32_t running = 0;
  int ok = count == visible;
  for (uint32_t k = 0; k < count; ++k) {
    ok = ok && cmds[k].firstIndex == running && cmds[k].instanceCount == 1 && (cmds[k].indexCount == 36 || cmds[k].indexCount == 18);
    running += cmds[k].indexCount;
  }
  ok = ok && running == index_total && model[12] == pos[0] && model[15] == 1.0f;
  /* Batched draws (extension): with DEVICE buffers — the renderer's own, imported with mip_import_external_fd — the frame above
   * is followed, without a wait, by
   *     MipBatchOutputs b = { sizeof b, MIP_OUT_DEVICE | MIP_OUT_ASYNC, batch_cmds, batch_count, instance_ids, NULL, batch_model };
   *     mip_batch_draws(ctx, &frame, visible_bitmap_dev, &b);
   * and drawn with vkCmdDrawIndexedIndirectCount(cb, batch_cmds, 0, batch_count, 0, 2 * n_meshes, 20); the vertex shader reads
   * entity_id = instance_ids[gl_InstanceIndex] (the depth pass: model = batch_model[gl_InstanceIndex]). This host owns no
   * device memory, so it only checks that the entry point links from C and refuses host pointers without harming the context. */
  MipBatchOutputs batch;
  memset(&batch, 0, sizeof batch);
  batch.struct_size = sizeof batch;
  batch.flags = MIP_OUT_HOST;
  batch.batch_cmds = cmds;
  batch.batch_count = &count;
  batch.instance_ids = bitmap;
  ok = ok && mip_batch_draws(ctx, &frame, bitmap, &batch) == MIP_ERR_INVALID_ARGUMENT && mip_instance_count(ctx) == N;
  /* Cluster culling for several views (extension): after mip_set_geometry and mip_build_clusters, and behind a mip_run_views
   * that wrote the views' bitmaps, with no wait,
   *     MipClusterViewOutputs cv = { sizeof cv, MIP_OUT_DEVICE | MIP_OUT_ASYNC, cluster_cmds, cmd_stride, 0, cmd_counts, NULL };
   *     mip_cull_clusters_views(ctx, frames, bitmaps_dev, n_views, &policy, &cv);
   * and per view vkCmdDrawIndexedIndirectCount(cb, cluster_cmds, v * cmd_stride * 20, cmd_counts, v * 4, cmd_stride, 20).
   * Here: the struct and the entry point link from C, and host pointers are refused without harming the context. */
  MipClusterViewOutputs cluster_views;
  const uint32_t* view_bitmaps[1] = {NULL};
  MipLodPolicy policy;
  memset(&policy, 0, sizeof policy);
  policy.struct_size = sizeof policy;
  memset(&cluster_views, 0, sizeof cluster_views);
  cluster_views.struct_size = sizeof cluster_views;
  cluster_views.flags = MIP_OUT_HOST;
  cluster_views.cluster_cmds = cmds;
  cluster_views.cmd_stride = 1;
  cluster_views.cmd_counts = &count;
  ok = ok && mip_cull_clusters_views(ctx, &frame, view_bitmaps, 1, &policy, &cluster_views) == MIP_ERR_INVALID_ARGUMENT &&
       mip_instance_count(ctx) == N;
  /* The visible-cluster lists of several views (extension): the same place in a frame, with
   *     MipClusterViewListOutputs lv = { sizeof lv, MIP_OUT_DEVICE | MIP_OUT_ASYNC, entries, entry_stride, 0, entry_counts, draw_args, NULL };
   *     mip_list_clusters_views(ctx, frames, bitmaps_dev, n_views, &policy, &lv);
   * and per view vkCmdDrawIndirect(cb, draw_args, 16 * v, 1, 16): firstInstance = v * entry_stride is the view's first entry.
   * Here: the struct and the entry point link from C, and host pointers are refused without harming the context. */
  MipClusterViewListOutputs list_views;
  memset(&list_views, 0, sizeof list_views);
  list_views.struct_size = sizeof list_views;
  list_views.flags = MIP_OUT_HOST;
  list_views.cluster_entries = cmds;
  list_views.entry_stride = 1;
  list_views.entry_counts = &count;
  ok = ok && mip_list_clusters_views(ctx, &frame, view_bitmaps, 1, &policy, &list_views) == MIP_ERR_INVALID_ARGUMENT &&
       mip_instance_count(ctx) == N;
  /* ... and with a depth pyramid per view (extension): `occs` is a host array of n_views host pointers, NULL for a view that
   * is tested against its planes alone; V pyramids built with mip_build_depth_pyramid need no wait in front of
   *     MipClusterViewOccludedListOutputs lo = { sizeof lo, MIP_OUT_DEVICE | MIP_OUT_ASYNC, entries, entry_stride, 0, entry_counts, draw_args, NULL, hidden };
   *     mip_list_clusters_views_occluded(ctx, frames, bitmaps_dev, occs, n_views, &policy, &lo);
   * Here: the struct and the entry point link from C, and host pointers are refused without harming the context. */
  MipClusterViewOccludedListOutputs list_occluded;
  const MipOcclusion* view_occs[1] = {NULL};
  memset(&list_occluded, 0, sizeof list_occluded);
  list_occluded.struct_size = sizeof list_occluded;
  list_occluded.flags = MIP_OUT_HOST;
  list_occluded.cluster_entries = cmds;
  list_occluded.entry_stride = 1;
  list_occluded.entry_counts = &count;
  ok = ok && mip_list_clusters_views_occluded(ctx, &frame, view_bitmaps, view_occs, 1, &policy, &list_occluded) == MIP_ERR_INVALID_ARGUMENT &&
       mip_instance_count(ctx) == N;
  /* Per-triangle masks on the visible-cluster list (extension): behind a run that wrote `visible_bitmap_dev`, with no wait,
   *     MipClusterTriangleListOutputs tl = { sizeof tl, MIP_OUT_DEVICE | MIP_OUT_ASYNC, entries, masks, entry_capacity, 0, entry_count, draw_args, NULL };
   *     mip_list_cluster_triangles(ctx, &frame, visible_bitmap_dev, &policy, NULL, NULL, &tl);
   * and ONE vkCmdDrawIndirect(cb, draw_args, 0, 1, 16): the shader reads entries[gl_InstanceIndex] and masks[gl_InstanceIndex]
   * and emits the triangles whose bit is set. Here: the struct and the entry point link from C, and host pointers are refused
   * without harming the context. */
  MipClusterTriangleListOutputs triangle_list;
  uint64_t mask_word = 0;
  memset(&triangle_list, 0, sizeof triangle_list);
  triangle_list.struct_size = sizeof triangle_list;
  triangle_list.flags = MIP_OUT_HOST;
  triangle_list.cluster_entries = cmds;
  triangle_list.triangle_masks = &mask_word;
  triangle_list.entry_capacity = 1;
  triangle_list.entry_count = &count;
  ok = ok && mip_list_cluster_triangles(ctx, &frame, bitmap, &policy, NULL, NULL, &triangle_list) == MIP_ERR_INVALID_ARGUMENT &&
       mip_instance_count(ctx) == N;
  printf("C_SMOKE %s instances=%d visible=%u commands=%u index_total=%u checksum=%08x\n", ok ? "OK" : "BAD", N, visible, count,
         index_total, sum);
  mip_destroy(ctx);
  mip_destroy(NULL); /* idempotent on NULL */
  return ok ? 0 : 1;
}
