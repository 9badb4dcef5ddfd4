"""Option launch_units_max and the stats launch_units_max and split_launches, without a device:
the range, the value in force, the counter of a fresh context, the binding's documentation, and
the source of the five launchers that read the option (in the style of test_layout_contract)."""
import os
import re

import pytest

import rsmi
from test_layout_contract import _body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
DEFAULT = (1 << 24) - 1


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_range_and_value_in_force():
    with rsmi.Codec(10, 4) as c:
        assert c.stat("launch_units_max") == DEFAULT
        for v in (1, 2, 4097, DEFAULT - 1, DEFAULT):
            c.set_option("launch_units_max", v)
            assert c.stat("launch_units_max") == v
        c.set_option("launch_units_max", 7)
        c.set_option("launch_units_max", 0)   # 0 restores the default
        assert c.stat("launch_units_max") == DEFAULT
        c.set_option("launch_units_max", 5)
        for v in (-1, DEFAULT + 1, 1 << 31, -(1 << 40)):
            with pytest.raises(rsmi.RsmiError) as e:
                c.set_option("launch_units_max", v)
            assert e.value.code == rsmi.ErrInvalidArg
            assert c.stat("launch_units_max") == 5   # a refused value changes nothing


def test_counter_of_a_fresh_context_and_unknown_keys():
    with rsmi.Codec(4, 2) as c:
        assert c.stat("split_launches") == 0
        c.set_option("launch_units_max", 3)
        assert c.stat("split_launches") == 0      # setting the option launches nothing
        assert c.stat("coalesced_calls") == 0
        for key in ("split_launch", "launch_units", "launch_units_max ", "", "nope"):
            assert c.stat(key) == -1, key
        with pytest.raises(rsmi.RsmiError) as e:
            c.set_option("launch_units", 3)
        assert e.value.code == rsmi.ErrInvalidArg


def test_documented_where_the_other_options_are():
    doc = rsmi.Codec.set_option.__doc__
    assert "launch_units_max" in doc and "split_launches" in doc and "waves_per_cu" in doc
    with open(os.path.join(ROOT, "include", "rsmi.h")) as f:
        header = f.read()
    options = header[header.index("/* Options:"):header.index("int rsmi_set_option(")]
    assert '"launch_units_max"' in options
    stats = header[header.index("/* Counters:"):header.index("long rsmi_get_stat(")]
    assert '"launch_units_max"' in stats and '"split_launches"' in stats
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert "`launch_units_max`" in design and "`split_launches`" in design


READS = "uint64_t(c->opt_launch_units_max) / "
COUNTS = "c->split_launches.fetch_add(1, std::memory_order_relaxed);"


def test_the_five_sites_read_the_option():
    """Each launcher forms its blocks per launch from the option, counts every launch of its loop
    behind the launch, and holds no 2^31 of its own."""
    plan = _body(src("rsmi_core.cpp"), "launch_plan")
    tiles = _body(src("rsmi_verify.cpp"), "launch_stripe_tiles")
    plan_crc = _body(src("rsmi_crc.cpp"), "launch_plan_crc")
    scrub = _body(src("rsmi_scrub.cpp"), "launch_scrub")
    mixed = _body(src("rsmi_mixed.cpp"), "launch_mixed")
    per = {"tpb": (plan, tiles), "upb": (plan_crc, scrub)}
    for unit, bodies in per.items():
        for body in bodies:
            line = "const uint64_t max_blocks = std::max<uint64_t>(1, %s%s);" % (READS, unit)
            assert body.count(line) == 1 and body.count("max_blocks =") == 1, (unit, body[:60])
            assert body.count("+= max_blocks) {") == 1
    assert ("const uint64_t seg = std::min<uint64_t>(std::max<uint64_t>(1, %stpb), uint64_t(1) << 22);" % READS) in mixed
    assert "for (uint64_t s0 = b0; s0 < b0 + nb; s0 += seg) {" in mixed
    for name, body in (("plan", plan), ("tiles", tiles), ("plan_crc", plan_crc), ("scrub", scrub), ("mixed", mixed)):
        assert body.count("opt_launch_units_max") == 1, name
        assert "(uint64_t(1) << 31) /" not in body and "<< 31) /" not in body, name
        # one counted launch per site: the launch inside the loop, the counter right behind it
        assert body.count(COUNTS) == 1, name
        at = body.index(COUNTS)
        launch = body[body.rindex("HIP_TRY(hipLaunchKernel(", 0, at):at]
        assert launch.startswith("HIP_TRY(hipLaunchKernel(fn, ") and launch.count(";") == 1, (name, launch)
        assert re.fullmatch(r"HIP_TRY\(hipLaunchKernel\(fn, .*\)\);( // [^;]*)? ", launch), (name, launch)
    # a table is one launch: the table forms decline a group over the cap, no flag is disarmed for it
    for body in (plan, plan_crc):
        assert body.count("if (tb && nblocks > max_blocks) return RSMI_ERR_INVALID_ARG;") == 1
        assert "nblocks > max_blocks)" not in body.replace("if (tb && nblocks > max_blocks) return", "")


def test_the_option_is_stored_and_handed_to_the_lanes():
    impl = src("rsmi_impl.hpp")
    assert "constexpr uint64_t kLaunchUnitsDefault = (uint64_t(1) << 24) - 1;" in impl
    assert 'static_assert(kLaunchUnitsDefault * kWG < (uint64_t(1) << 32), "a unit launch stays below 2^32 threads");' in impl
    assert "std::atomic<long> opt_launch_units_max{long(rsmi::impl::kLaunchUnitsDefault)};" in impl
    assert "std::atomic<long> split_launches{0};" in impl
    core = " ".join(src("rsmi_core.cpp").split())
    assert ('} else if (!std::strcmp(key, "launch_units_max")) { '
            "if (value < 0 || value > long(kLaunchUnitsDefault)) return RSMI_ERR_INVALID_ARG; "
            "c->opt_launch_units_max.store(value ? value : long(kLaunchUnitsDefault));") in core
    coal = src("rsmi_coalesce.cpp")
    assert "x->opt_launch_units_max.store(c->opt_launch_units_max.load());" in coal
    assert 'if (!std::strcmp(key, "launch_units_max")) return c->opt_launch_units_max.load();' in coal
    assert 'if (!std::strcmp(key, "split_launches")) {' in coal
