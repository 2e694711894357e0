// The protocol of a scorer over the member store (gc_ens_reserve): what gc_ensemble.hip, gc_spectrum.hip, gc_events.hip
// and gc_derive.hip share on the host.  An entry of theirs reads as: validation (ready checks, store_complete,
// check_peer), take_truth, its buffer groups, a Bracket around its launches, the readback.  Host code only.
#pragma once
#include "gc_handle.h"

namespace gci {

// floats of one member field [G, B, c_out] / of one conditioning array [G, B, c_in]
inline size_t field_len(const gc_handle* h) { return (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out; }
inline size_t cond_len(const gc_handle* h) { return (size_t)h->hg.G * h->cfg.batch * h->cfg.c_in; }

// through the pinned staging buffer of the noise upload ([G, B, c_out] floats), in pieces where the payload is longer
inline int store_upload(gc_handle* h, void* dev, const void* src, size_t bytes) {
  return staged_upload_bytes(h, h->pin_noise, field_len(h) * sizeof(float), dev, src, bytes);
}

// every slot of `store` has been pushed since its gc_ens_reserve; `prefix`: "" or "source "
inline int store_complete(gc_handle* h, const gc_handle* store, const char* prefix = "") {
  for (int i = 0; i < store->ens_members; ++i)
    if (!store->ens_filled[(size_t)i])
      return fail(h, GC_ERR_STATE, std::string(prefix) + "member slot " + std::to_string(i) + " has not been pushed");
  return GC_OK;
}

// a failure inside a call made on another handle is reported on the handle the caller asked
inline int relay(gc_handle* h, gc_handle* o, int rc, const char* who) {
  if (rc && o != h) h->err = std::string(who) + " handle: " + o->err;
  return rc;
}

// The truth the store of `owner` is scored against: `truth` is uploaded into the owner's buffer (made on first use) and
// stays there; null means the one already there.  `owner` is `h`, or the source handle of gc_ens_derive.
inline int take_truth(gc_handle* h, gc_handle* owner, const float* truth, const char* entry) {
  if (!truth) {
    if (owner->has_ens_truth) return GC_OK;
    return fail(h, GC_ERR_STATE, std::string("no truth on the ") + (owner == h ? "device" : "source handle") + " (pass one to " + entry + ")");
  }
  const size_t n = field_len(owner);
  int rc;
  if (!owner->d_ens_truth && (rc = relay(h, owner, dev_alloc(owner, &owner->d_ens_truth, n), "source"))) return rc;
  if ((rc = relay(h, owner, staged_upload(owner, owner->pin_noise, owner->d_ens_truth, truth, n), "source"))) return rc;
  owner->has_ens_truth = true;
  return GC_OK;
}

// The handle on the other side of a call, `who` ("source", "other"): same device, a graph, the same G and batch, and
// of the channel counts those the caller names -- c_in equal to this handle's, c_out equal to `c_out` (< 0: any).
inline int check_peer(gc_handle* h, const gc_handle* o, const char* who, bool c_in, int c_out = -1, const char* c_out_name = "c_out") {
  const std::string the = std::string("the ") + who + " handle ";
  if (o->device != h->device) return fail(h, GC_ERR_INVALID_ARGUMENT, the + "is on another device");
  if (!o->has_graph || o->hg.G != h->hg.G || o->cfg.batch != h->cfg.batch || (c_in && o->cfg.c_in != h->cfg.c_in) ||
      (c_out >= 0 && o->cfg.c_out != c_out))
    return fail(h, GC_ERR_INVALID_ARGUMENT, the + "has other dimensions (G, batch" + (c_in ? ", c_in" : "") + (c_out >= 0 ? std::string(", ") + c_out_name : "") + ")");
  return GC_OK;
}

// `then` goes on behind everything enqueued on `first` so far
inline int order_behind(gc_handle* h, Event& ev, hipStream_t first, hipStream_t then) {
  GC_HIP(h, hipEventRecord(ev.e, first));
  GC_HIP(h, hipStreamWaitEvent(then, ev.e, 0));
  return GC_OK;
}

// `work` enqueues on the PEER's stream (in front of that handle's next sample) something that writes this handle's
// store.  The two streams are ordered by events, both ways: the store is no longer being read when the work starts, and
// is complete before this handle's stream goes on.
template <typename F>
int on_peer_stream(gc_handle* h, gc_handle* peer, F&& work) {
  int rc;
  if ((rc = order_behind(h, h->ev_ens_free, h->stream, peer->stream)) || (rc = work())) return rc;
  return order_behind(h, h->ev_ens_done, peer->stream, h->stream);
}

}  // namespace gci
