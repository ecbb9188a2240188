"""What the compiler made of the two forms of the compile-time robot's collision walk in the persistent STOMP kernel
(csrc/mpb_geom.h, waypoint_cost_grid_model<..., UNROLLED>; csrc/kernel_resources.json, written by build()): the one-field
instantiations take the walk with its group loop unrolled and must hold it in registers; the chained-field instantiations
keep the rolled loop and with it the scratch they had before the unrolled form existed."""
import json

import pytest

PANDA = 1                                    # PandaModel::ID
FORMS = [(dch, nb, inj) for dch in (14, 7) for nb in (1, 2) for inj in (False, True)]
# scratch [B per lane] of stomp_fused_kernel<DCH, 1, NB, INJ, true> in a build of the parent commit (rolled walk everywhere)
CHAINED_SCRATCH_PARENT = {(14, 1, False): 0, (14, 1, True): 0, (14, 2, False): 0, (14, 2, True): 48,
                          (7, 1, False): 0, (7, 1, True): 0, (7, 2, False): 16, (7, 2, True): 36}


@pytest.fixture(scope='module')
def resources():
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    with open(build.RESOURCES) as fh:
        return json.load(fh)


def _kernel(resources, dch, nb, inj, chain):
    prefix = '_Z18stomp_fused_kernelILi%dELi%dELi%dELb%dELb%dEE' % (dch, PANDA, nb, inj, chain)
    hits = [v for k, v in resources.items() if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, len(hits))
    return hits[0]


@pytest.mark.parametrize('dch,nb,inj', FORMS)
def test_one_field_forms_hold_the_unrolled_walk_in_registers(resources, dch, nb, inj):
    r = _kernel(resources, dch, nb, inj, False)
    assert r['scratch'] == 0 and r['vgpr_spill'] == 0, r
    assert r['vgprs'] + r.get('agprs', 0) <= 128, r


@pytest.mark.parametrize('dch,nb,inj', FORMS)
def test_chained_forms_keep_the_scratch_of_the_rolled_walk(resources, dch, nb, inj):
    r = _kernel(resources, dch, nb, inj, True)
    assert r['scratch'] == CHAINED_SCRATCH_PARENT[(dch, nb, inj)], r
