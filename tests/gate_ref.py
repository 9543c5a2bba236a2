"""The temporal gate of `build_graph(start_frames=, max_gap=)`, in plain torch on the CPU -- TEST INFRASTRUCTURE.

Applied to a DENSE cross-camera list (what `build_graph` without the gate, or oracle.graph_oracle.topology, returns): the
reference's commented-out statements (inference.py:420-441), literally -- per edge the distance of the two tracklets' start
frames, kept where it is below the gap.

The composed rule "gate, then k" needs no code of its own: with pg = select(starts, edge_index, max_gap),
    pg[knn_ref.select(attr_cos[pg], edge_index[:, pg], cams, k)]
(the gated list holds both directions of every pair, which knn_ref.reverse_positions requires)."""
import torch


def select(start_frames, edge_index, max_gap):
    """Kept dense positions (ascending, int64 tensor)."""
    s = [int(v) for v in torch.as_tensor(start_frames).tolist()]            # Python integers: no overflow at any frame
    rows, cols = torch.as_tensor(edge_index).tolist()
    kept = []
    for e, (row, col) in enumerate(zip(rows, cols)):
        start1, start2 = s[row], s[col]
        dist = start2 - start1 if start1 <= start2 else start1 - start2
        if dist < max_gap:
            kept.append(e)
    return torch.tensor(kept, dtype=torch.int64)
