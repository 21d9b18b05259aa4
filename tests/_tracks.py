"""The bookkeeping of landmark identities (include/ekfvio.h, "landmark identities and the tracks that ended") as a pure-Python model, no
device: a list of (id, born) in landmark order, a counter that never goes back, appends at the end, removals that keep the order."""
import numpy as np


class TrackModel:
    def __init__(self):
        self.rows = []      # (id, born) per landmark, in landmark order
        self.next_id = 0    # survives reset()
        self.total_ended = 0

    def append(self, k, stamp):
        """k new landmarks at the end: ids next_id .. next_id + k - 1, all born at `stamp` (NaN: no stamp yet)."""
        self.rows += [(self.next_id + j, float(stamp)) for j in range(int(k))]
        self.next_id += int(k)

    def remove(self, mask):
        """Takes out the landmarks with a nonzero mask entry; returns the ended rows [(id, born, index_before)] in landmark order."""
        mask = np.asarray(mask).astype(bool).reshape(-1)
        assert mask.shape[0] == len(self.rows), (mask.shape, len(self.rows))
        ended = [(i, b, row) for row, ((i, b), m) in enumerate(zip(self.rows, mask)) if m]
        self.rows = [r for r, m in zip(self.rows, mask) if not m]
        self.total_ended += len(ended)
        return ended

    def replace(self, n, stamp):
        """ekfvio_set_state: the landmark set is replaced, n fresh ids in order."""
        self.rows = []
        self.append(n, stamp)

    def reset(self):
        """ekfvio_reset: no landmarks, the counter goes on, the ended total starts over."""
        self.rows = []
        self.total_ended = 0

    @property
    def ids(self):
        return np.array([r[0] for r in self.rows], np.int64)

    @property
    def born(self):
        return np.array([r[1] for r in self.rows], np.float64)


def ended_arrays(ended):
    """(ids int64, born float64, index_before int32) of what TrackModel.remove returned."""
    return (np.array([e[0] for e in ended], np.int64), np.array([e[1] for e in ended], np.float64), np.array([e[2] for e in ended], np.int32))
