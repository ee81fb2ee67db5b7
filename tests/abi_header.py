"""What the ABI tests (tests/test_abi.py, tests/test_abi_png16.py) know about the headers' C types: how a scalar parameter
type reads in _lib's signature tables, and how wide the element of a device pointer is."""
import re

SCALARS = {"uint64_t": "u64", "uint32_t": "u32", "size_t": "size", "int": "int"}
POINTEE_BYTES = {"uint8_t": 1, "uint32_t": 4, "uint64_t": 8, "fdh_png_info": 4, "fdh_resume_point": 4}


def pointee(param):
    """The type a pointer parameter points to, or None for a scalar one."""
    if "*" not in param and "[" not in param:
        return None
    return re.match(r"(?:const )?(\w+)", param).group(1)
