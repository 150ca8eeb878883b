/* fmx_post_check.c -- the argument and state checks of the posterior accumulator (fmx_post_*, fmx_group_post_*) from plain C:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude examples/fmx_post_check.c -Llibfm_amd -lfmx -Wl,-rpath,$PWD/libfm_amd \
 *       -Wl,-rpath-link,/opt/rocm/lib -o fmx_post_check
 * Needs no device: without one fmx_create fails with FMX_E_HIP and every entry point must refuse the NULL handle / group with
 * FMX_E_ARG instead of touching it.  With a device the same calls are made on a handle whose slots are empty: FMX_E_ARG for
 * the bad arguments, FMX_E_STATE for the slot that was never uploaded.  Exits non-zero on the first surprise.
 */
#include <stdio.h>
#include <string.h>
#include "fmx.h"

static int failures = 0;
#define WANT(call, code) do { int rc_ = (call); if (rc_ != (code)) { fprintf(stderr, "%s -> %d, expected %d\n", #call, rc_, (code)); failures++; } } while (0)

int main(void) {
  fmx_config c;
  memset(&c, 0, sizeof(c));
  c.num_attribute = 100; c.num_factor = 2; c.k0 = 1; c.k1 = 1; c.task = FMX_TASK_CLASSIFICATION;
  c.min_target = -1; c.max_target = 1; c.device = -1; c.shard_world = 1;
  fmx_handle h = NULL;
  fmx_post_opts bad_flags = {5u, 0u, 1u, 0u};
  fmx_post_stats st;
  fmx_eval_ex ev;
  double vec[4];
  uint64_t draws = 0;
  const int rc = fmx_create(&c, &h);
  if (rc != FMX_OK) {
    WANT(rc, FMX_E_HIP);
    printf("no device (%s): the NULL handle\n", fmx_last_error(NULL));
    h = NULL;
  }
  /* the group calls never see a group here */
  WANT(fmx_group_post_begin(NULL, 0, NULL), FMX_E_ARG);
  WANT(fmx_group_post_accumulate(NULL, 0, &st), FMX_E_ARG);
  WANT(fmx_group_post_evaluate_ex(NULL, 0, FMX_POST_ALL, &ev), FMX_E_ARG);
  WANT(fmx_group_post_get(NULL, 0, FMX_POST_ALL, vec, &draws), FMX_E_ARG);
  WANT(fmx_group_post_end(NULL, 0), FMX_E_ARG);
  if (!h) {
    WANT(fmx_post_begin(NULL, 0, NULL), FMX_E_ARG);
    WANT(fmx_post_begin(NULL, 0, &bad_flags), FMX_E_ARG);
    WANT(fmx_post_accumulate(NULL, 0, NULL), FMX_E_ARG);
    WANT(fmx_post_accumulate(NULL, 0, &st), FMX_E_ARG);
    WANT(fmx_post_evaluate_ex(NULL, 0, FMX_POST_ALL, &ev), FMX_E_ARG);
    WANT(fmx_post_evaluate_ex(NULL, 0, 3u, NULL), FMX_E_ARG);
    WANT(fmx_post_get(NULL, 0, FMX_POST_LATE, vec, &draws), FMX_E_ARG);
    WANT(fmx_post_get(NULL, -1, 7u, NULL, NULL), FMX_E_ARG);
    WANT(fmx_post_end(NULL, 0), FMX_E_ARG);
  } else {
    WANT(fmx_post_begin(h, 0, &bad_flags), FMX_E_ARG);
    WANT(fmx_post_begin(h, -1, NULL), FMX_E_ARG);
    WANT(fmx_post_begin(h, FMX_MAX_SLOTS, NULL), FMX_E_ARG);
    WANT(fmx_post_begin(h, 0, NULL), FMX_E_STATE);                 /* never uploaded */
    WANT(fmx_post_accumulate(h, 0, &st), FMX_E_STATE);
    WANT(fmx_post_evaluate_ex(h, 0, FMX_POST_ALL, NULL), FMX_E_ARG);
    WANT(fmx_post_evaluate_ex(h, 0, 3u, &ev), FMX_E_ARG);
    WANT(fmx_post_evaluate_ex(h, 0, FMX_POST_ALL, &ev), FMX_E_STATE);
    WANT(fmx_post_get(h, 0, 3u, vec, &draws), FMX_E_ARG);
    WANT(fmx_post_get(h, 0, FMX_POST_THIS, vec, &draws), FMX_E_STATE);
    WANT(fmx_post_end(h, 0), FMX_E_STATE);
    WANT(fmx_destroy(h), FMX_OK);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
