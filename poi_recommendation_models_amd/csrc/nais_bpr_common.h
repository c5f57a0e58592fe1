// nais_bpr_common.h -- shared by nais_bpr.hip and nais_bpr_train.hip (not ABI).
#pragma once

#include "nais_internal.h"

static inline int nais_bpr_check_params(const nais_bpr_params_t* q) {
  if (!q) return nais_internal_fail(NAIS_E_INVALID, "NULL params");
  if (q->embed_dim < 1 || q->embed_dim > 256)
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "BPR embed_dim must be 1..256");
  if (q->num_pois < 1 || q->num_users < 1) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (q->num_pois >= (int64_t(1) << 24))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "BPR num_pois must be below 2^24");
  if (!q->embed_user || !q->embed_item)
    return nais_internal_fail(NAIS_E_INVALID, "NULL parameter pointer");
  return NAIS_OK;
}
