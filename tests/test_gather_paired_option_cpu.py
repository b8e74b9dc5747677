"""F2N_OPT_GATHER_PAIRED is numbered from F2N_OPT2_FIRST, behind the first option table (keys 0 .. 12,
which stays closed: key 13 is rejected): reachable by name, a switch with values 0 and 1, default 0, and
nothing else in or around the second range is a key."""
INVALID = -1


def test_gather_paired_option_is_a_switch_in_the_second_range(capi):
    first, later = capi.option_keys(), capi.later_option_keys()
    assert later == {"GATHER_PAIRED": 64} and not set(later) & set(first)
    assert min(later.values()) > max(first.values()) + 1
    c = capi.lib().cdll
    key = later["GATHER_PAIRED"]
    assert c.f2n_get_option(key) == 0                      # vertex-parity order is the default
    with capi.option("GATHER_PAIRED", 1):
        assert c.f2n_get_option(key) == 1
        assert all(c.f2n_get_option(k) == 0 for k in first.values())   # no slot shared with the first table
    assert c.f2n_get_option(key) == 0
    assert c.f2n_set_option(key, 2) == INVALID and c.f2n_set_option(key, -1) == INVALID
    for bad in (len(first), key - 1, key + 1):
        assert c.f2n_set_option(bad, 0) == INVALID and c.f2n_get_option(bad) == INVALID
