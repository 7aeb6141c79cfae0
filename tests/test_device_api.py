"""The device stepper API (include/turtle_amd_device.h) where no GPU is needed: the header, the test
kernels and the example compile on their own with -Wall -Werror, the Stepping-based traverse kernel
costs its caller no occupancy and no scratch against k_traverse, the host calls fail
loudly without a device, and the ISA record of the move is there."""
import os
import re

import pytest

import turtle_amd as TA
from turtle_amd import binding as Bn

import device_loops as DL

ROOT = DL.ROOT


@pytest.mark.parametrize("source", ["include/turtle_amd_device.h", "tests/c/device_loops.hip",
                                    "examples/own_kernel.hip"])
def test_compiles_alone_with_only_include_on_the_path(tmp_path, source):
    extra = ["-x", "hip"] if source.endswith(".h") else []
    DL.compile_object(os.path.join(ROOT, source), str(tmp_path / "unit.o"), extra)


def resources(remarks):
    """{function name: {vgpr, scratch, occupancy}} from -Rpass-analysis=kernel-resource-usage"""
    out, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (.*?)\s*\[-Rpass", line)
        if not m:
            continue
        key, _, value = m.group(1).strip().partition(":")
        key, value = key.strip(), value.strip()
        if key == "Function Name":
            name = value
            out[name] = {}
        elif name and key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
            out[name][key.split(" ")[0]] = int(value)
    return out


# waves per SIMD of k_traverse's instance of the same mode and arithmetic, and the
# scratch allowed: none, or GENERIC's 40 bytes (k_walk's, the call frame of d_project)
WAVES = {("ONE_MAP", "fast"): (4, 0), ("ONE_STACK", "fast"): (3, 0), ("ONE_MAP", "strict"): (2, 0),
         ("ONE_STACK", "strict"): (2, 0), ("GENERIC", "fast"): (2, 40), ("GENERIC", "strict"): (2, 40)}
MODES = {"GENERIC": 0, "ONE_MAP": 1, "ONE_STACK": 2}


def test_stepping_costs_no_occupancy_and_no_scratch(tmp_path):
    remarks = DL.compile_object(DL.SOURCE, str(tmp_path / "loops.o"),
                                ["-Rpass-analysis=kernel-resource-usage"])
    table = resources(remarks)
    for (mode, math), (waves, scratch) in WAVES.items():
        # traverse_trip<MODE, MATH>: Li<mode>ELi<math>E in the mangled name
        tag = "traverse_tripILi%dELi%dE" % (MODES[mode], DL.MATH[math])
        rows = [v for k, v in table.items() if tag in k]
        assert len(rows) == 1, (tag, list(table))
        print(mode, math, rows[0])
        assert rows[0]["Occupancy"] >= waves, (mode, math, rows[0])
        assert rows[0]["ScratchSize"] <= scratch, (mode, math, rows[0])


def test_view_acquire_without_a_device_fails_loudly():
    st = TA.Stepper()
    st.add_flat(0.0)
    if TA.device_count() > 0:   # (a device is visible here: then the call works)
        with st.view() as v:
            assert len(v) == Bn.view_layout()[1]
        st.destroy()
        return
    with pytest.raises(TA.TurtleError) as e:
        with st.view():
            pass
    assert e.value.name == "LIBRARY_ERROR" and "no CPU path" in str(e.value)
    st.destroy()


def test_view_arguments_are_checked_before_anything_else():
    import ctypes as C
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    buf = C.create_string_buffer(1024)
    for args, name in (((None, buf, C.c_size_t(Bn.view_layout()[1])), "BAD_ADDRESS"),
                       ((st.h, None, C.c_size_t(Bn.view_layout()[1])), "BAD_ADDRESS"),
                       ((st.h, buf, C.c_size_t(Bn.view_layout()[1] + 8)), "DOMAIN_ERROR")):
        with pytest.raises(TA.TurtleError) as e:
            Bn._check(L.turtle_amd_stepper_view_acquire(*args))
        assert e.value.name == name
    with pytest.raises(TA.TurtleError) as e:   # releasing what was not acquired: an error, not a crash
        Bn._check(L.turtle_amd_stepper_view_release(st.h))
    assert e.value.name == "DOMAIN_ERROR"
    st.destroy()


def test_header_and_library_agree_on_the_view():
    version, size = Bn.view_layout()
    assert (DL.lib().loops_view_version(), DL.lib().loops_view_size()) == (version, size)


def test_isa_record_reports_no_differing_instruction():
    text = open(os.path.join(ROOT, "profiles", "device_api_isa.txt")).read()
    rows = [l for l in text.splitlines() if re.search(r"\s(identical|DIFFERS)\s+sgpr=", l)]
    assert len(rows) >= 275 and not [l for l in rows if "DIFFERS" in l]
    assert "outside the kernels (rest.s): identical" in text
    m = re.search(r"(\d+) kernels, (\d+) differ", text)
    assert m and int(m.group(1)) == len(rows) and int(m.group(2)) == 0
    for kernel in ("k_traverse<", "k_walk<", "k_trace<", "k_step<", "k_bisect<", "k_cross<", "k_resample<"):
        assert any(l.startswith(kernel) for l in rows), kernel
