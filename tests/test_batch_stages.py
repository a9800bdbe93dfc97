"""CPU checks of the host stages the batched single-FOWT and array entry points share
(raft/model.py): the record of a batch's further sea states and a case as one FOWT sees it."""
import numpy as np

from raft.model import FurtherSeaStates, Model

CASES = [dict(wave_heading=10, wave_spectrum="JONSWAP", wave_period=9, wave_height=3, wave_gamma=0),
         dict(wave_heading=[0, 30, -20], wave_spectrum=["JONSWAP", "unit", "JONSWAP"], wave_period=[10, 11, 12],
              wave_height=[4, 5, 6], wave_gamma=[0, 1, 2.5]),
         dict(wave_heading=[45, 90], wave_spectrum=["still", "constant"], wave_period=[7, 8], wave_height=[1, 2],
              wave_gamma=[3.3, 0])]


def record(cases):
    seas = [Model._case_sea_states(c) for c in cases]
    return FurtherSeaStates(seas, np.array([len(s[0]) for s in seas], dtype=np.int64))


def test_further_sea_states_of_counts_1_3_2():
    ext = record(CASES)
    assert ext.pairs == [(1, 1), (1, 2), (2, 1)]
    assert ext.case.tolist() == [1, 1, 2] and ext.case.dtype == np.int64
    assert ext.sea.tolist() == [1, 2, 1] and ext.sea.dtype == np.int64
    assert ext.nwm == 3
    assert ext.heading == [30.0, -20.0, 90.0]
    assert ext.spectrum == ["unit", "JONSWAP", "constant"]
    assert ext.Hs == [5.0, 6.0, 2.0]
    assert ext.Tp == [11.0, 12.0, 8.0]
    assert ext.gamma == [1.0, 2.5, 0.0]
    assert np.array_equal(ext.betas, np.array([30.0, -20.0, 90.0]) * 0.017453292519943295)


def test_further_sea_states_of_counts_1_1_is_empty():
    ext = record([CASES[0], dict(CASES[0], wave_heading=-5)])
    assert ext.pairs == [] and ext.nwm == 1
    assert ext.case.shape == (0,) and ext.sea.shape == (0,) and ext.betas.shape == (0,)
    assert ext.heading == ext.spectrum == ext.Hs == ext.Tp == ext.gamma == []


def old_copy(case, i):
    """The reduction as the three statics loops each spelled it before they shared _fowt_case."""
    ci = dict(case)
    if isinstance(case.get("wind_speed"), list):
        ci["wind_speed"] = case["wind_speed"][i]
    return ci


def test_fowt_case():
    scalar = dict(wind_speed=8.0, wind_heading=20, turbine_status="operating", wave_heading=[0, 30])
    listed = dict(scalar, wind_speed=[10.0, 6.0])
    for i in range(2):
        assert Model._fowt_case(scalar, i) == old_copy(scalar, i) == scalar
        assert Model._fowt_case(listed, i) == old_copy(listed, i) == dict(scalar, wind_speed=[10.0, 6.0][i])
    got = Model._fowt_case(listed, 1)
    got["wave_heading"] = 0                      # a copy: the caller's case keeps its entries
    assert listed["wind_speed"] == [10.0, 6.0] and listed["wave_heading"] == [0, 30]
    assert "wind_speed" not in Model._fowt_case(dict(wave_heading=0), 0)
