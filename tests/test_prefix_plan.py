"""BatchDecodeEngine._prefix_plan (models/decoder.py): who of a pass's pending requests starts from the captured
prefix rows, who computes them and who waits, decided from host state alone -- driven here with no device."""


def _engine(prefix, ready=False):
    from libsplinter_amd.models.decoder import BatchDecodeEngine
    eng = BatchDecodeEngine.__new__(BatchDecodeEngine)  # the host bookkeeping only: no model, no cache
    eng.pend = {}
    eng._pfx_ids, eng._pfx_ready, eng._pfx_donor = list(prefix), ready, None
    return eng


def _pending(eng, slot, carries, off=0):
    eng.pend[slot] = [list(eng._pfx_ids) + [7] if carries else [9, 9], off, 0, carries]


def test_lowest_carrying_slot_is_the_donor_and_the_others_are_held():
    eng = _engine([1, 2, 3, 4])
    _pending(eng, 3, True)
    _pending(eng, 1, True)
    _pending(eng, 0, False)  # does not carry the prefix: neither donor nor held
    _pending(eng, 5, True)
    assert eng._prefix_plan() == ([], 1, [3, 5])
    assert eng._pfx_donor == 1
    # the donor stays the donor while it is pending, whatever lands in a lower slot and wherever it has got to
    eng.pend[1][1] = 2
    _pending(eng, 0, True)
    assert eng._prefix_plan() == ([], 1, [0, 3, 5])


def test_released_donor_hands_over_to_the_lowest_carrying_slot_at_offset_0():
    eng = _engine([1, 2, 3, 4])
    for slot in (2, 4, 6):
        _pending(eng, slot, True)
    assert eng._prefix_plan() == ([], 2, [4, 6])
    eng.pend[2][1] = 2
    del eng.pend[2]          # BatchDecodeEngine.release of a pending donor
    eng._pfx_donor = None
    assert eng._prefix_plan() == ([], 4, [6])
    assert eng.pend[4][1] == 0


def test_after_capture_a_carrying_request_at_offset_0_is_a_hit_once():
    eng = _engine([1, 2, 3, 4], ready=True)
    _pending(eng, 0, True)
    _pending(eng, 1, False)
    _pending(eng, 2, True, off=4)  # already past the prefix: an ordinary segment
    assert eng._prefix_plan() == ([0], None, [])
    eng.pend[0][1] = 4             # prefill moves a hit to offset R
    assert eng._prefix_plan() == ([], None, [])


def test_no_prefix_or_nobody_carrying_plans_nothing():
    eng = _engine([])
    _pending(eng, 0, False)
    assert eng._prefix_plan() == ([], None, [])
    eng = _engine([1, 2])
    _pending(eng, 0, False)
    assert eng._prefix_plan() == ([], None, []) and eng._pfx_donor is None
