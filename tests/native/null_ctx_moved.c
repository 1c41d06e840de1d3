/* The entry points of ta_api_walls.hip, ta_api_sparse.hip and ta_api_exchange.hip with a NULL context (tests/test_sanitized_host.py
 * builds and runs this against the host-sanitized library; no device is needed): each must answer TA_EINVAL, and the program prints
 * the text it leaves in ta_last_error. */
#include <stdio.h>
#include <stdint.h>
#include "tissue_scan.h"

static int bad = 0;
static void said(const char* name, int rc) {
    printf("%s: %d %s\n", name, rc, ta_last_error());
    if (rc != TA_EINVAL) bad = 1;
}

int main(void) {
    ta_ctx* c = NULL;
    int rc = ta_ctx_create(0, &c);                       /* (fails cleanly where there is no device) */
    if (rc == TA_OK && ta_ctx_destroy(c) != TA_OK) return 2;
    if (rc != TA_OK && c != NULL) return 3;
    int64_t n = 0; uint32_t u = 0, v = 0; int flag = 0; double ms = 0.0; void* p = NULL; void* q = NULL;
    uint32_t pairs[2]; int32_t coords[3]; uint64_t block[8];
    said("ta_wall_voxels_count", ta_wall_voxels_count(NULL, &n));
    said("ta_wall_voxels_get", ta_wall_voxels_get(NULL, pairs, coords, &ms));
    said("ta_wall_voxels_get_by_pair", ta_wall_voxels_get_by_pair(NULL, pairs, coords, &ms));
    said("ta_wall_medians", ta_wall_medians(NULL, 10, &n, &ms));
    said("ta_wall_medians_get", ta_wall_medians_get(NULL, pairs, &u, coords));
    said("ta_volume_max_label", ta_volume_max_label(NULL, &u));
    said("ta_volume_label_census", ta_volume_label_census(NULL, &u, &v));
    said("ta_label_census_get", ta_label_census_get(NULL, &u));
    said("ta_volume_compact_labels", ta_volume_compact_labels(NULL, NULL, 0, &u));
    said("ta_volume_is_compact", ta_volume_is_compact(NULL, &flag, &u));
    said("ta_volume_rerank", ta_volume_rerank(NULL));
    said("ta_volume_uncompact", ta_volume_uncompact(NULL));
    said("ta_accumulators_reduced", ta_accumulators_reduced(NULL));
    said("ta_accumulators_device", ta_accumulators_device(NULL, &p, &q, &u));
    said("ta_adjacency_device", ta_adjacency_device(NULL, &p, &q, &n));
    said("ta_adjacency_export", ta_adjacency_export(NULL, block, block, 1));
    said("ta_adjacency_merge", ta_adjacency_merge(NULL, block, block, 0));
    said("ta_adjacency_pack", ta_adjacency_pack(NULL, block, 1));
    said("ta_adjacency_pack_shared", ta_adjacency_pack_shared(NULL, block, 1));
    said("ta_adjacency_merge_blocks", ta_adjacency_merge_blocks(NULL, block, 1, 1));
    return bad;
}
