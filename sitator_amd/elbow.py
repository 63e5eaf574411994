"""``index_of_elbow`` (reference: ``sitator/util/elbow.py``): the point of a sorted curve farthest from the straight line
between its first and last points."""
import numpy as np


def index_of_elbow(points):
    """The index of the "elbow" in ``points``, after sorting them in descending order: the point with the largest distance
    to the line from ``(0, points[0])`` to ``(n - 1, points[n - 1])``.  Pretty approximate; long flat tails pull it to the right."""
    curve = np.sort(np.asarray(points, dtype=np.float64))[::-1]
    xy = np.column_stack([np.arange(len(curve)), curve])
    line = xy[-1] - xy[0]
    line /= np.linalg.norm(line)
    from_first = xy - xy[0]
    along = np.outer(np.sum(from_first * line, axis=1), line)
    return np.argmax(np.linalg.norm(from_first - along, axis=1))
