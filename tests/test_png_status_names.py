"""The PNG status values have two vocabularies, the FDH_PNG_STATUS_* macros of include/fdeflate_hip.h and the PNG_*
constants of fdeflate_amd.api: they must name the same values (csrc/png_common.h ties the kernels to the header with
static_asserts, this ties the Python layer to it)."""
import os
import re

from fdeflate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_statuses():
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    return {name: int(value) for name, value in re.findall(r"^#define FDH_PNG_STATUS_([A-Z0-9_]+) (\d+)u$", text, flags=re.M)}


def test_header_and_api_name_the_same_png_status_values():
    header = _header_statuses()
    # what the PNG specification's pipeline can report: reconstruction 0..3, the scan 1..6, the decode steps 7..11
    assert sorted(header.values()) == [0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    for name, value in header.items():
        assert getattr(api, "PNG_" + name) == value, name
    in_api = {k[4:] for k in vars(api) if re.fullmatch(r"PNG_(OK|BAD_\w+|SKIPPED|SCAN_[A-Z_]+|OTHER_GEOMETRY|COMP_SLOT_TOO_SMALL|INDEX_OUTSIDE_PALETTE)", k)}
    assert in_api - {"SCAN_STATUS_NAMES"} == set(header)
    assert (header["OK"], header["BAD_FILTER_TYPE"], header["BAD_SIZES"], header["SKIPPED"]) == (0, 1, 2, 3)
    assert (header["OTHER_GEOMETRY"], header["COMP_SLOT_TOO_SMALL"], header["INDEX_OUTSIDE_PALETTE"], header["BAD_PLTE"], header["BAD_TRNS"]) == (7, 8, 9, 10, 11)


def test_api_flags_are_the_headers():
    """Every FLAG_* / PNG_FLAG_* of api is the header's FDH_FLAG_* / FDH_PNG_FLAG_* of the same name (the header may
    define flags that api does not name)."""
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    header = {name: int(value, 16) for name, value in re.findall(r"^#define FDH_((?:PNG_)?FLAG_[A-Z0-9_]+)\s+(0x[0-9A-Fa-f]+)u\b", text, flags=re.M)}
    named = {k: v for k, v in vars(api).items() if re.fullmatch(r"(PNG_)?FLAG_[A-Z0-9_]+", k)}
    assert len(named) >= 22 and {"FLAG_IGNORE_ADLER32", "FLAG_NO_LANES", "PNG_FLAG_IGNORE_CRC", "PNG_FLAG_ADAM7"} <= set(named)
    for name, value in named.items():
        assert header[name] == value, name


def test_scan_status_names_list_the_scan_values_in_order():
    header = _header_statuses()
    names = api.PNG_SCAN_STATUS_NAMES
    assert names[0] == "Ok" and len(names) == 7
    for value, name in enumerate(names[1:], start=1):
        macro = "SCAN_" + re.sub(r"(?<!^)([A-Z])", r"_\1", name).upper()  # "NoSignature" -> "SCAN_NO_SIGNATURE"
        assert header[macro] == value, (name, macro)
        assert getattr(api, "PNG_" + macro) == value
    assert sorted(v for k, v in header.items() if k.startswith("SCAN_")) == list(range(1, 7))
