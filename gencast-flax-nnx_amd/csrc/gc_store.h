// The two host protocols of the units over the member store (gc_ens_reserve).  Host code only.
//
// Scoring a store (gc_ens_score, gc_ens_spectrum, gc_ens_event_score, gc_ens_fss_score, gc_ens_order_*, gc_ens_clim_score,
// gc_ens_efi_score, gc_ens_energy_score, gc_ens_variogram_score, gc_ens_tail_score, gc_ens_region_score):
//   1. the state checks, one `||` chain of need_graph / need(plan) / need_store / need_out / store_complete / need_weights /
//      check_peer in the order THIS entry reports them (the orders differ, and tests pin them);
//   2. hipSetDevice, take_truth;
//   3. its buffers: sized_for(a KeyedGroup of the handle, its sizes, the buffers) (gc_handle.h);
//   4. timed(its Meter, the launches, the read-backs): begin, launches, end, read-backs, synchronise, device time, ++calls;
//   5. what is its own: how `invalid` is formed from what came back, which outputs are optional.
// Filling a store from a source handle (gc_ens_derive, gc_ens_band, gc_ens_feature; gc_ens_window_emit, which has no
// source, uses own_truth_buffer / store_rewritten / fill_close alone):
//   1. need_source, need_graph, its plan;
//   2. fill_open: the source checks, take_truth into the SOURCE, this handle's truth buffer, the entry's work buffers,
//      order_behind the source's stream, store_rewritten;
//   3. timed(...) as above;  4. fill_close: every slot filled, a truth on the device.
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

// ---- the state checks, one message each ------------------------------------------------------------------------------------
inline int need(gc_handle* h, bool ok, const char* msg) { return ok ? GC_OK : fail(h, GC_ERR_STATE, msg); }
inline int need_graph(gc_handle* h) { return need(h, h->has_graph, "gc_set_graph must be called first"); }
inline int need_store(gc_handle* h) { return need(h, h->ens_members != 0, "no member store (gc_ens_reserve)"); }
inline int need_weights(gc_handle* h) { return need(h, h->has_ens_w, "no node weights (gc_ens_set_node_weight)"); }
// a required output (or input) pointer of the caller
inline int need_out(gc_handle* h, bool given) { return given ? GC_OK : fail(h, GC_ERR_INVALID_ARGUMENT, "null argument"); }
inline int need_source(gc_handle* h, const gc_handle* src) {
  return src && src != h ? GC_OK : fail(h, GC_ERR_INVALID_ARGUMENT, "the source must be another handle");
}

// ---- the timed body ----------------------------------------------------------------------------------------------------
// every launch through launch(h, KC_PACK, ...), in order, up to the first that fails
template <typename... F>
int launch_each(gc_handle* h, F&&... f) {
  int rc = GC_OK;
  ((rc = rc ? rc : launch(h, gc::KC_PACK, f)), ...);
  return rc;
}

// `n` elements device to host on the handle's stream; the uint64_t form copies the device's unsigned long long as they lie
template <typename T>
int read_back(gc_handle* h, T* dst, const T* src, size_t n) {
  GC_HIP(h, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return GC_OK;
}
inline int read_back(gc_handle* h, uint64_t* dst, const unsigned long long* src, size_t n) {
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counts are copied out as they lie");
  GC_HIP(h, hipMemcpyAsync(dst, src, n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  return GC_OK;
}

// The device work of one call on the handle's stream, between the unit's two events: `launches` enqueues it, `readbacks`
// the copies to the host behind it; on return they have landed, m.device_us is the time between the events and the call
// is counted.
template <typename L, typename R>
int timed(gc_handle* h, Meter& m, L&& launches, R&& readbacks) {
  hipStream_t s = h->stream;
  int rc;
  GC_HIP(h, m.time.begin(s));
  if ((rc = launches())) return rc;
  GC_HIP(h, m.time.end(s));
  if ((rc = readbacks())) return rc;
  GC_HIP(h, hipStreamSynchronize(s));
  GC_HIP(h, m.time.microseconds(&m.device_us));
  ++m.calls;
  return GC_OK;
}
inline int no_readbacks() { return GC_OK; }

// ---- filling the store of `h` from the store of `src` ------------------------------------------------------------------------
// the truth buffer of a handle whose truth is written on the device
inline int own_truth_buffer(gc_handle* h) { return h->d_ens_truth ? GC_OK : dev_alloc(h, &h->d_ens_truth, field_len(h)); }

// the store is about to be written as a whole: what was made from its old contents is no longer of this store
inline void store_rewritten(gc_handle* h) {
  h->evt_scored = false;
  h->has_ens_fields = false;
  h->ord_ready = false;
  h->efi_fields = 0;
}

// The opening, behind need_source and the entry's plan check: the source has c_out == c_src of the plan and a complete
// store of as many members as this one; `truth` goes into the SOURCE's truth buffer (as gc_ens_score(src, truth, ..)
// would put it); this handle's truth buffer; `work_buffers` makes the entry's own; then the handle's stream goes on
// behind the source's, on which the source's store and truth are complete.
template <typename F>
int fill_open(gc_handle* h, gc_handle* src, int c_src, const float* truth, const char* entry, Event& ev, F&& work_buffers) {
  int rc;
  if ((rc = check_peer(h, src, "source", false, c_src, "c_out == c_src of the plan")) || (rc = need_store(h)) ||
      (rc = need(h, src->ens_members != 0, "no member store on the source handle (gc_ens_reserve)")) ||
      (rc = need(h, src->ens_members == h->ens_members, "the two member stores hold different numbers of members")) ||
      (rc = store_complete(h, src, "source ")))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, src, truth, entry)) || (rc = own_truth_buffer(h)) || (rc = work_buffers()) ||
      (rc = order_behind(h, ev, src->stream, h->stream)))
    return rc;
  store_rewritten(h);
  return GC_OK;
}

// The close: every slot holds a field of this call, and so does the truth buffer.
inline void fill_close(gc_handle* h) {
  std::fill(h->ens_filled.begin(), h->ens_filled.end(), 1);
  h->has_ens_truth = true;
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
