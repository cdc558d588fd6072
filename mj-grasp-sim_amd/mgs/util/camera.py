"""Camera helpers (reference: mgs/util/camera.py:87-112)."""
import math

import numpy as np


def fibonacci_sphere(total_num, i):
    """the i-th of total_num points spread over the unit sphere by the golden
    angle: y runs from +1 (i = 0) to -1 (i = total_num - 1), the point turns by
    pi (3 - sqrt 5) about y per index.  The reference divides by total_num - 1,
    so fewer than two points is an error here rather than a ZeroDivisionError."""
    if total_num < 2:
        raise ValueError("fibonacci_sphere needs total_num >= 2 (the spacing is 2 / (total_num - 1))")
    y = 1 - (2.0 * i / (total_num - 1))
    radius = math.sqrt(max(0.0, 1.0 - y * y))
    theta = math.pi * (3.0 - math.sqrt(5.0)) * i
    return np.array([math.cos(theta) * radius, y, math.sin(theta) * radius])
