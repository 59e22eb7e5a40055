"""tests/feature_state_rectify_cases.py through the C ABI: every sequence on a context of its own, the flags read back through what the API
shows (the refusals of gbuffer_read, history_mark_read and history_rectify).  The same table runs through csrc/flx_feature_state.h on the CPU
in tests/test_feature_state_rectify.py.  No call here is refused by anything but an argument check on the host."""
import numpy as np
import pytest
import common
import feature_state_rectify_cases as fs
from test_gpu_feature_state import Run as Base, _refuses, _refusal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    d = common.mixed_material_scene()
    d.tris.setflags(write=False)
    return d


class Run(Base):
    def event(self, e):
        g, k = self.g, e[0]
        if k == "mark": g.history_mark()
        elif k == "rectify": g.history_rectify()
        elif k == "rectify_bad": g.history_rectify(radius=0)
        elif k == "wf_reset": g.wf_reset()
        elif k == "write_pixels": g.write_pixels(0, np.ones((self.blank.shape[0], 4), np.float32))
        elif k == "refused":
            before = self.flags()
            with pytest.raises(RuntimeError, match=e[2]):
                self.event(e[1])
            assert self.flags() == before, "a refused call changed the state"
        else: super().event(e)

    def flags(self):
        """(T0, Mk, MkMom, Live); the rectify that answers Live runs last (where it runs it may change the mark's values, never the flags)"""
        g = self.g
        T0 = int(not _refuses(lambda: g.gbuffer_read(0), "the slot holds no G-buffer"))
        Mk = int(not _refuses(g.history_mark_read, "no mark"))
        why = _refusal(lambda: g.history_mark_read(moments=True))
        assert not why or "no mark" in why or "holds no moments" in why, why
        why2 = _refusal(g.history_rectify)
        g.finish()
        assert not why2 or "no mark" in why2 or "no G-buffer of the mark's size" in why2, why2
        return (T0, Mk, int(not why), int(not why2))


@pytest.mark.parametrize("case", fs.CASES, ids=[c["name"] for c in fs.CASES])
def test_sequence(scene, case):
    r = Run(scene)
    try:
        for e in case["events"]:
            r.event(e)
        got = r.flags()
    finally:
        r.g.close()
    print(case["name"], got)
    assert got == case["expect"]
