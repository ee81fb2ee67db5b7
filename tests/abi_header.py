"""What the ABI tests (tests/test_abi*.py) share: how a header's prototypes are read, how a scalar parameter type reads in
_lib's signature tables, how wide the element of a device pointer is, and the comparison of a table with its header."""
import re

SCALARS = {"uint64_t": "u64", "uint32_t": "u32", "size_t": "size", "int": "int"}
POINTEE_BYTES = {"uint8_t": 1, "uint32_t": 4, "uint64_t": 8, "fdh_png_info": 4, "fdh_resume_point": 4}


def pointee(param):
    """The type a pointer parameter points to, or None for a scalar one."""
    if "*" not in param and "[" not in param:
        return None
    return re.match(r"(?:const )?(\w+)", param).group(1)


def declared_prototypes(header_path):
    """{symbol: (result, [parameter, ...])} as the header spells them, comments and preprocessor lines taken out."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for result, name, params in re.findall(r"([^;{}]*?)\b(fdh_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        params = [" ".join(p.split()) for p in params.split(",")]
        protos[name] = (" ".join(result.split()).replace('extern "C"', "").strip(), [] if params == ["void"] else params)
    return protos


def check_table(header_path, table):
    """The header's prototypes, after holding `table` (one of _lib's) to them: the same symbols, the parameter count, the
    class of every parameter and of the result, the element width of every device pointer and the place of the stream.
    A miscounted table entry would be undefined behaviour at the call, not an error."""
    from fdeflate_amd import _lib
    protos = declared_prototypes(header_path)
    assert set(protos) == set(table)
    for name, (result, params) in protos.items():
        t_result, t_params = table[name]
        if "*" in result:
            assert t_result == ("str" if result == "const char *" else "host"), name
        else:
            assert t_result == ("void" if result == "void" else SCALARS[result]), name
        assert len(t_params) == len(params), name
        for pos, (token, param) in enumerate(zip(t_params, params)):
            where = "%s, parameter %d (%s)" % (name, pos, param)
            pointed = pointee(param)
            if pointed is None:
                assert token == SCALARS[param.split()[0]], where
            elif token in _lib.DEVICE_WIDTH:
                assert param.count("*") == 1 and "[" not in param, where
                assert _lib.DEVICE_WIDTH[token] == POINTEE_BYTES[pointed], where
            else:
                assert token == ("stream" if param == "void *hip_stream" else "host"), where   # exempt from the widths
        assert ("stream" in t_params) == (t_params[-1:] == ("stream",)) == (params[-1:] == ["void *hip_stream"]), name
    return protos
