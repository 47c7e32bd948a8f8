"""Two kernels, one cell: iso_derived_chain and iso_population_eval interpolate the same packed table at the same 257
points (one full workgroup plus one lane) and give the same bits, NaN positions included; both helpers also assert that
the guard margins around the outputs are untouched."""
import pytest

from tests import _derived_gpu as dg, _derived_twin as dtw, _grid_interp as gi, _population_twin as ptw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Q", gi.QS)
def test_derived_and_population_kernels_give_the_same_bits(Q):
    tab = ptw.tables(Q, 1)
    cols, ax3 = tab[0], tab[1]
    rows = gi.points()
    out, _ = dg.device(gi.as_chain(rows), dtw.ROW_MAJOR, 1, gi.N, cols, ax3, gi.COMPS)
    got = ptw.device(ptw.DeviceTables(tab), *gi.as_systems(rows), want=("cols_out",))
    gi.assert_same_cell(out, got["cols_out"])
