/* cgo_shape_sparse.c — bgn_sparse_lincomb_batch and bgn_sparse_lincomb_batch_dev used the way go/bgn_amd.go's
 * SparseLinCombBatch and SparseLinCombBatchDev use them, from plain C (what cgo compiles), deterministic and blinded: the
 * device form with row_ptr, col and w back to back in ONE device array.  Exit 0 iff every call returned the expected
 * bytes, which tests/test_cgo_shape_sparse.py computes with the oracle and hands in as hex:
 *   cgo_shape_sparse P_HEX N_HEX L P_WIRE Q_WIRE  LEVEL D NROWS NNZ ROW_MAX W_BITS CT_HEX IDX_HEX WANT_HEX  R_HEX WANT_BLINDED_HEX
 * IDX_HEX: the nrows + 1 + 2 nnz words of row_ptr, col and w in the byte order of the host. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bgn_amd.h"

static size_t unhex(const char* s, uint8_t** out) {
  size_t n = strlen(s) / 2, i;
  *out = (uint8_t*)malloc(n ? n : 1);
  for (i = 0; i < n; ++i) {
    unsigned v;
    sscanf(s + 2 * i, "%2x", &v);
    (*out)[i] = (uint8_t)v;
  }
  return n;
}

int main(int argc, char** argv) {
  uint8_t *p, *n, *Pw, *Qw, *ct, *idx_b, *want[2], *r, *out;
  uint32_t* idx;
  const uint32_t *rp, *col;
  const int32_t* w;
  void *d_ct, *d_idx, *d_r, *d_out;
  size_t p_len, n_len, E, d, nrows, nnz, row_max, nvec, nin, nb, ni;
  bgn_ctx* ctx = NULL;
  int rc, level, w_bits, blind, failures = 0;
  if (argc != 17) return 2;
  p_len = unhex(argv[1], &p);
  n_len = unhex(argv[2], &n);
  unhex(argv[4], &Pw);
  unhex(argv[5], &Qw);
  rc = bgn_ctx_create(&ctx, p, p_len, n, n_len, strtoull(argv[3], NULL, 10), Pw, Qw, 1, 0);
  if (rc) {
    printf("bgn_ctx_create: %d %s\n", rc, bgn_last_error());
    return 3;
  }
  E = 2 * bgn_fp_bytes(ctx);
  level = atoi(argv[6]);
  d = (size_t)strtoull(argv[7], NULL, 10);
  nrows = (size_t)strtoull(argv[8], NULL, 10);
  nnz = (size_t)strtoull(argv[9], NULL, 10);
  row_max = (size_t)strtoull(argv[10], NULL, 10);
  w_bits = atoi(argv[11]);
  nin = unhex(argv[12], &ct);
  nvec = nin / E / d;
  nb = nvec * nrows * E;
  ni = 4 * (nrows + 1 + 2 * nnz);
  if (unhex(argv[13], &idx_b) != ni || unhex(argv[14], &want[0]) != nb || unhex(argv[15], &r) != nvec * nrows * n_len ||
      unhex(argv[16], &want[1]) != nb)
    return 2;
  idx = (uint32_t*)malloc(ni);
  memcpy(idx, idx_b, ni);
  rp = idx;
  col = idx + nrows + 1;
  w = (const int32_t*)(idx + nrows + 1 + nnz);
  out = (uint8_t*)malloc(nb);
  d_ct = bgn_dev_alloc(ctx, nin);
  d_idx = bgn_dev_alloc(ctx, ni);
  d_r = bgn_dev_alloc(ctx, nvec * nrows * n_len);
  d_out = bgn_dev_alloc(ctx, nb);
  if (!d_ct || !d_idx || !d_r || !d_out || bgn_dev_upload(ctx, d_ct, ct, nin) || bgn_dev_upload(ctx, d_idx, idx, ni) ||
      bgn_dev_upload(ctx, d_r, r, nvec * nrows * n_len))
    return 4;
  for (blind = 0; blind < 2; ++blind) {
    memset(out, 0, nb);
    rc = bgn_sparse_lincomb_batch(ctx, nvec, nrows, d, nnz, row_max, level, ct, rp, col, w, w_bits, blind ? r : NULL,
                                  blind ? n_len : 0, out);
    if (rc || memcmp(out, want[blind], nb)) failures++;
    memset(out, 0, nb);
    rc = bgn_sparse_lincomb_batch_dev(ctx, nvec, nrows, d, nnz, row_max, level, (const uint8_t*)d_ct, (const uint32_t*)d_idx,
                                      (const uint32_t*)d_idx + nrows + 1, (const int32_t*)d_idx + nrows + 1 + nnz, w_bits,
                                      blind ? (const uint8_t*)d_r : NULL, blind ? n_len : 0, (uint8_t*)d_out, NULL);
    if (!rc) rc = bgn_dev_download(ctx, out, d_out, nb);
    if (rc || memcmp(out, want[blind], nb)) failures++;
  }
  bgn_dev_free(ctx, d_ct);
  bgn_dev_free(ctx, d_idx);
  bgn_dev_free(ctx, d_r);
  bgn_dev_free(ctx, d_out);
  bgn_ctx_destroy(ctx);
  printf("cgo_shape_sparse: %zu results, %d failures\n", nvec * nrows, failures);
  return failures ? 1 : 0;
}
