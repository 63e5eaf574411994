"""GPU: operators and chains of operators on frame shards against the single-rank pipeline (tests/shard_ref.py), on the
real kernels.  A thread, a ``ThreadComm`` end and a trajectory per rank, every context on GPU 0; the single-rank run of a
case is finished (and its contexts released) before the ranks start, so a case holds a trajectory context per rank - five
at the most - besides what an operator opens and closes inside one call (the scratch context of the smoothing, the
``PBCCalculator`` of a merge).

The single-rank answers are the oracle's (``jump_analysis``, ``jumps``, ``assign_to_last_known_site``,
``running_windowed_mode`` on the whole array) and the single-rank operator run; everything is compared with exact
equality.  tests/test_shard_chains.py runs the same checks on a numpy stand-in, where there is no GPU."""
import pytest

from tests import shard_ref as S

pytestmark = pytest.mark.gpu

LAB, K, CUTS = S.designed()
INPUTS = [("designed/%d" % n, LAB, K, CUTS[n]) for n in sorted(CUTS)] + [("seed%d" % s,) + S.random_case(s) for s in S.SEEDS]
IDS = [c[0] for c in INPUTS]
DESIGNED = INPUTS[:3]


@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_jump_analysis_on_shards(oracle, name, lab, k, cut):
    S.check_jump_analysis(oracle, lab, k, cut)


@pytest.mark.parametrize("unknown_as_jump", [False, True])
@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_jumps_on_shards(oracle, name, lab, k, cut, unknown_as_jump):
    S.check_jumps(oracle, lab, k, cut, unknown_as_jump)


@pytest.mark.parametrize("threshold", S.ASSIGN_THRESHOLDS)
@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_assign_to_last_known_site_on_shards(oracle, name, lab, k, cut, threshold):
    S.check_assign(oracle, lab, k, cut, threshold)


@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_occupancy_on_shards(oracle, name, lab, k, cut):
    S.check_occupancy(oracle, lab, k, cut)


@pytest.mark.parametrize("remove", [False, True])
@pytest.mark.parametrize("mode", S.SMOOTH_MODES)
@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_smoothing_on_shards(oracle, name, lab, k, cut, mode, remove):
    S.check_smoothing(oracle, lab, k, cut, mode, remove)


@pytest.mark.parametrize("name,lab,k,cut", DESIGNED, ids=IDS[:3])
def test_smoothing_leaves_the_inputs_labels_resident(oracle, name, lab, k, cut):
    S.check_input_labels_stay_resident(oracle, lab, k, cut)


@pytest.mark.parametrize("chain", [S.chain_1, S.chain_2], ids=["chain1", "chain2"])
@pytest.mark.parametrize("name,lab,k,cut", DESIGNED, ids=IDS[:3])
def test_chains_on_shards(oracle, name, lab, k, cut, chain):
    S.check_chain(oracle, chain, lab, k, cut)
