// Host-only view of K2's 64-bit state word as the encoder lays it out
// (csrc/encode.cpp "host ports ... as state bits", csrc/antiaff.cpp): built to
// lib/libsrstateview.so together with the HIP-free encoder objects, so
// tests/test_state_word_reference.py can prove the bit positions of
// tests/state_word.py without a GPU.  Not part of libsrplanner.so or the ABI:
// the library carries its own copy of sr_snapshot_create / sr_snapshot_add_pod
// / sr_snapshot_destroy, and the snapshot passed in must come from it.
//   make -C k8s-spot-rescheduler_amd tools
#include <string>

#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"

extern "C" {

// One fresh encode of `cands` on `snap`.  Outputs: *swap_mask; status[n_cand]
// the host status of every input candidate (SR_CAND_FALLBACK, SR_CAND_EMPTY,
// anything else: planned on the device); for every active pod q < *n_active
// word 3 of its pod record (the state bits it sets) in pod_bits[q] and its
// index into cand_pods (relative to cand_pod_off[0]) in pod_src[q].  Both pod
// arrays hold cap_pods entries; more active pods than that is an error.
sr_status sr_state_word_view(const sr_cluster* cluster, const sr_snapshot* snap, const sr_candidates* cands,
                             uint64_t* swap_mask, int32_t* status, uint64_t* pod_bits, int32_t* pod_src,
                             int32_t cap_pods, int32_t* n_active) {
  sr::EncoderCache cache;
  sr::Workload w;
  std::string err;
  const sr_status st = sr::encode_workload(&cache, snap, cluster, cands, &w, &err);
  if (st != SR_OK) return st;
  const int32_t n = static_cast<int32_t>(w.pod_src.size());
  if (n > cap_pods) return SR_ERR_INVALID_ARG;
  *swap_mask = w.swap_mask;
  *n_active = n;
  for (int32_t i = 0; i < cands->n_cand; ++i) status[i] = w.status_host[i];
  for (int32_t q = 0; q < n; ++q) {
    pod_bits[q] = w.pod_rec[static_cast<size_t>(q) * 6 + 3];
    pod_src[q] = w.pod_src[q] - w.pod_base;
  }
  return SR_OK;
}

}  // extern "C"
