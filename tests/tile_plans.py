"""Hand-built tile plans for the FFT path (test infrastructure, no device access).

On the periodic whole-DEM context a tile loads its input modulo the DEM, and sc_match accepts any plan whose tiles
cover the core: neither V == T - span nor T <= n is required.  So a tile of any supported size - 64 to 4096 on either
axis, in any number - can be put on a small DEM, and one float64 oracle stack of that DEM can serve every kernel class the
route of the FFT path (scarplet_amd/csrc/sc_fft_route.h) knows.  tests/test_tile_plans_host.py checks these plans on the host.
"""

SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


def min_tiles(n, span, T):
    """The smallest number of tiles of length ``T`` that cover ``n`` cells with a support of ``span`` + 1 cells."""
    if span >= T:
        raise ValueError("a support of %d cells does not fit a tile of %d" % (span + 1, T))
    return -(-n // (T - span))


def count_with_parity(n, span, T, at_least, odd):
    """The smallest tile count >= ``at_least`` that covers the axis and is odd (``odd``) or even."""
    nt = max(min_tiles(n, span, T), at_least)
    return nt if (nt % 2 == 1) == bool(odd) else nt + 1


def _axis(n, span, T, nt):
    if T not in SIZES:
        raise ValueError("tile length %r" % (T,))
    if span >= T:
        raise ValueError("a support of %d cells does not fit a tile of %d" % (span + 1, T))
    if nt is None:
        nt = min_tiles(n, span, T)
    if nt < 1:
        raise ValueError("tile count %r" % (nt,))
    V = min(T - span, -(-n // nt))
    if nt * V < n:
        raise ValueError("%d tiles of %d (%d valid cells each) do not cover %d cells" % (nt, T, V, n))
    if (nt - 1) * V >= n:
        raise ValueError("%d tiles of %d valid cells: the last one lies outside the %d cells" % (nt, V, n))
    return V, nt


def forced_plan(ny, nx, bbox, Ty, Tx, nty=None, ntx=None, group=1):
    """The fields of an sc_plan that puts ``nty`` x ``ntx`` tiles of ``Ty`` x ``Tx`` on the whole periodic ``ny`` x
    ``nx`` DEM for templates with the support box ``bbox`` = (pmin, pmax, qmin, qmax): non-circular axes with the origin
    _plan.Plan gives them (Py = pmax, Qx = qmax), V = min(T - span, ceil(n / nt)) valid cells per tile, the count
    defaulting to the smallest that covers the axis.  ValueError where the support does not fit the tile or the tiles
    do not cover the DEM."""
    pmin, pmax, qmin, qmax = bbox
    Vy, nty = _axis(ny, pmax - pmin, Ty, nty)
    Vx, ntx = _axis(nx, qmax - qmin, Tx, ntx)
    return dict(method=1, Ty=Ty, Tx=Tx, Vy=Vy, Vx=Vx, nty=nty, ntx=ntx, circ_y=0, circ_x=0, Py=pmax, Qx=qmax,
                group=group)


class ModelPlan(object):
    """The fields of forced_plan as the object tests/pipeline_model.py takes for a _plan.Plan."""

    def __init__(self, ny, nx, fields):
        self.ny, self.nx = ny, nx
        self.oy, self.ox = ny % 2, nx % 2
        self.core = (0, ny, 0, nx)
        for k, v in fields.items():
            setattr(self, k, v)
        self.circ_y, self.circ_x = bool(fields["circ_y"]), bool(fields["circ_x"])

    def tiles(self):
        """[(i0, j0, vy, vx, gi0, gj0)] as _plan.Plan.tiles() (and fft_prepare) lay them out."""
        out = []
        for ty in range(self.nty):
            i0 = ty * self.Vy
            for tx in range(self.ntx):
                j0 = tx * self.Vx
                out.append((i0, j0, min(self.Vy, self.ny - i0), min(self.Vx, self.nx - j0),
                            i0 + self.oy - self.Py, j0 + self.ox - self.Qx))
        return out
