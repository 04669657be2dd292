// forge_args.h -- what a leader-schedule launch carries (forge.h
// forge_schedule_item), the same for every lane: the expanded key (the reduced
// scalar and the public key bytes as given), the epoch nonce and
// ouro_leader_params.  Passed by value with the launch; every host copy is
// zeroed before the call returns (forge_api.cpp).  At global scope, so the
// kernel unit (its lane routines in a renamed namespace) and the host units
// name the same type.
#pragma once
#include <stdint.h>

struct OuroForgeSched {
  uint32_t x[8];
  uint32_t pk[8];
  uint32_t eta0[8];
  uint32_t have_eta0;  // 0: NeutralNonce
  uint32_t f_is_one;
  uint32_t ngen;
  uint32_t pad;
  uint64_t epoch_first_slot;
  uint64_t sigma_num, sigma_den;
  uint64_t act_log_lo;
  int64_t act_log_hi;
  uint64_t d_num, d_den;
  uint64_t asc_inv;
};
