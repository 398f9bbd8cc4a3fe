"""numpy reference for the radial camera model with l1, l2 estimated (test helper, no GPU).

distortion_ref.RadialOracle holds l1 and l2: columns 1 and 2 of its Jacobian are zero.  With the
mapper's "estimate the distortion" switch they are parameters like f, and since

    (u, v) = f d (x, y),  d = 1 + r2 (l1 + l2 r2),  r2 = x^2 + y^2,

the two columns are  d(u, v)/dl1 = f r2 (x, y)  and  d(u, v)/dl2 = f r2^2 (x, y),  at the same
normalized point (x, y) the oracle returns for the unit camera.  FreeRadialOracle is RadialOracle
plus those two columns, with the oracle's signatures, so tag_size_ref.solve (its `free` mask
already counts camera slots 1 and 2 as parameters of a free camera), tag_size_ref.SizedOracle
(x and y do not change with the tag-side scale, so neither do the columns) and loss_ref run on it
unchanged.
"""
import numpy as np

import distortion_ref


class FreeRadialOracle(distortion_ref.RadialOracle):
    """RadialOracle with the l1, l2 columns of the Jacobian filled in."""

    def residual_jacobian(self, cam, cap, tag, corners):
        cam = np.asarray(cam, np.float64)
        r, J = super().residual_jacobian(cam, cap, tag, corners)
        xy = self.oracle.residual(distortion_ref._UNIT_CAMERA, cap, tag, distortion_ref._ZERO_CORNERS).reshape(4, 2)
        r2 = np.sum(xy * xy, axis=1)[:, None]
        J = J.copy()
        J[:, 1] = (cam[0] * r2 * xy).reshape(8)
        J[:, 2] = (cam[0] * r2 * r2 * xy).reshape(8)
        return r, J


def zero_lens(arrays):
    """The problem's arrays with the camera's l1, l2 at zero: where an estimate starts."""
    return distortion_ref.with_distortion(arrays, (0.0, 0.0))
