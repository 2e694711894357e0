"""The float64 yardstick of the regional ensemble scores: per region, the reference of section 8c
(tests/verification_reference.py) on the region's node subset, and `invalid` likewise.

Test infrastructure only (the product never imports it).  `members` [M, G, B, C] and `truth` [G, B, C] are float32 (the
device's inputs), `w` [G], `node_bits` [G] uint32 (bit r set = the node belongs to region r).
"""
import numpy as np

from tests import verification_reference as VR


def region_nodes(node_bits, n_regions):
  """[R] index arrays: the nodes of every region, ascending."""
  bits = np.asarray(node_bits, dtype=np.uint32)
  return [np.flatnonzero((bits >> np.uint32(r)) & np.uint32(1)) for r in range(n_regions)]


def reference(members, truth, w, node_bits, n_regions):
  """-> dict: sums [R, B, C, 6], abs_sums [R, B, C, 6] (the scale of the tolerance), hist [R, B, C, M + 1] uint64,
  invalid [R] uint64 (the points of the region's nodes that were skipped).  An empty region has zeros."""
  members, truth, w = np.asarray(members), np.asarray(truth), np.asarray(w)
  parts = [VR.reference(members[:, idx], truth[idx], w[idx]) for idx in region_nodes(node_bits, n_regions)]
  return dict(sums=np.stack([p["sums"] for p in parts]), abs_sums=np.stack([p["abs_sums"] for p in parts]),
              hist=np.stack([p["hist"] for p in parts]), invalid=np.array([p["invalid"] for p in parts], np.uint64))


def sum_tolerance(ref, G, M):
  """|device - reference| <= (G + M^2 + 8) 2^-53 A_k per sum, A_k the reference's absolute sum over that region: the
  bound of section 8c (a region adds at most G terms per column)."""
  return (G + M * M + 8) * 2.0 ** -53 * ref["abs_sums"]
