/* fmx_snap_check.c -- the argument and state checks of the snapshot file calls (fmx_compact_save, fmx_compact_load,
 * fmx_snapshot_info, fmx_serve_open) from plain C:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude examples/fmx_snap_check.c -Llibfm_amd -lfmx -Wl,-rpath,$PWD/libfm_amd \
 *       -Wl,-rpath-link,/opt/rocm/lib -o fmx_snap_check
 * Needs no device: without one fmx_create fails with FMX_E_HIP and every entry point must refuse the NULL handle with FMX_E_ARG
 * instead of touching it; fmx_snapshot_info and the refusals of fmx_serve_open that come from the path and the file's header never
 * look for a device.  With a device the same calls are made on a handle without a snapshot: FMX_E_ARG for the bad arguments,
 * FMX_E_STATE for the save without a snapshot, and a file that is no snapshot is refused by name.  Exits non-zero on the first
 * surprise.
 */
#include <stdio.h>
#include <string.h>
#include "fmx.h"

static int failures = 0;
#define WANT(call, code) do { int rc_ = (call); if (rc_ != (code)) { fprintf(stderr, "%s -> %d, expected %d\n", #call, rc_, (code)); failures++; } } while (0)

int main(int argc, char **argv) {
  const char *junk = argc > 1 ? argv[1] : "fmx_snap_check.junk";     /* a file that is no snapshot: written here, removed at the end */
  fmx_config c;
  fmx_snap_info info;
  char err[128];
  fmx_handle h = NULL, s = (fmx_handle)&c;                             /* (s must come back NULL from every failed fmx_serve_open) */
  FILE *f = fopen(junk, "wb");
  if (!f) { fprintf(stderr, "cannot create %s\n", junk); return 1; }
  fputs("this is not a snapshot file; it is longer than a header all the same ......................................................"
        "..........................................................................................................................."
        ".....................................................................\n", f);
  fclose(f);
  memset(&c, 0, sizeof(c));
  c.num_attribute = 100; c.num_factor = 2; c.k0 = 1; c.k1 = 1; c.task = FMX_TASK_CLASSIFICATION;
  c.min_target = -1; c.max_target = 1; c.device = -1; c.shard_world = 1;
  /* no handle, no device */
  WANT(fmx_compact_save(NULL, junk, &info), FMX_E_ARG);
  WANT(fmx_compact_load(NULL, junk, &info), FMX_E_ARG);
  WANT(fmx_snapshot_info(NULL, &info, err, sizeof(err)), FMX_E_ARG);
  WANT(fmx_snapshot_info(junk, NULL, err, sizeof(err)), FMX_E_ARG);
  WANT(fmx_snapshot_info("no/such/file.snap", &info, err, sizeof(err)), FMX_E_ARG);
  WANT(fmx_snapshot_info(junk, &info, NULL, 0), FMX_E_ARG);
  WANT(fmx_snapshot_info(junk, &info, err, sizeof(err)), FMX_E_ARG);
  if (!strstr(err, "bad magic")) { fprintf(stderr, "fmx_snapshot_info says '%s', expected 'bad magic'\n", err); failures++; }
  WANT(fmx_snapshot_info(junk, &info, err, 4), FMX_E_ARG);             /* (a short buffer: truncated, not overrun) */
  WANT(fmx_serve_open(NULL, -1, &s, NULL), FMX_E_ARG);
  if (s) { fprintf(stderr, "fmx_serve_open(NULL path) left a handle\n"); failures++; }
  WANT(fmx_serve_open(junk, -1, NULL, NULL), FMX_E_ARG);
  s = (fmx_handle)&c;
  WANT(fmx_serve_open("no/such/file.snap", -1, &s, &info), FMX_E_ARG);
  if (s) { fprintf(stderr, "fmx_serve_open(missing file) left a handle\n"); failures++; }
  s = (fmx_handle)&c;
  WANT(fmx_serve_open(junk, -1, &s, &info), FMX_E_ARG);
  if (s || !strstr(fmx_last_error(NULL), "bad magic")) { fprintf(stderr, "fmx_serve_open(junk): handle %p, '%s'\n", (void *)s, fmx_last_error(NULL)); failures++; }
  {
    const int rc = fmx_create(&c, &h);
    if (rc != FMX_OK) {
      WANT(rc, FMX_E_HIP);
      printf("no device (%s): the NULL handle only\n", fmx_last_error(NULL));
      h = NULL;
    }
  }
  if (h) {
    WANT(fmx_compact_save(h, NULL, &info), FMX_E_ARG);
    WANT(fmx_compact_load(h, NULL, &info), FMX_E_ARG);
    WANT(fmx_compact_save(h, junk, &info), FMX_E_STATE);               /* no snapshot was taken */
    WANT(fmx_compact_save(h, junk, NULL), FMX_E_STATE);
    WANT(fmx_compact_load(h, "no/such/file.snap", &info), FMX_E_ARG);
    WANT(fmx_compact_load(h, junk, NULL), FMX_E_ARG);
    if (!strstr(fmx_last_error(h), "bad magic")) { fprintf(stderr, "fmx_compact_load says '%s'\n", fmx_last_error(h)); failures++; }
    WANT(fmx_compact_predict(h, 0, (double *)&info), FMX_E_STATE);     /* and the refused load left no snapshot behind */
    WANT(fmx_destroy(h), FMX_OK);
  }
  remove(junk);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
