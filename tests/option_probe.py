"""The deterministic probe behind test_option_table_cpu.py: what the public option surface of a libmlimgsynth_amd.so answers.

For every option a fresh context takes a fixed list of values through mlis_option_set_str and, where the option takes one int,
double, uint64 or string, a second fresh context takes a list through the variadic mlis_option_set.  After each call the probe notes
an outcome: [return code, mlis_errstr_get, error handler calls, mlis_option_get's return code, the value it gives] (the value read
through a 16-byte buffer; floats as float32 bit patterns).  It also notes mlis_option_get's return code for every id in 0..255 and
what setting an id that is no option answers.

To keep the fixture small the outcome is written without loss: "{}" stands for the value just given where the error text quotes it
or the getter returns it, None for an error text the call left as it was, "=" for a getter value the call left as it was; and per
option only the outcomes that differ from its most frequent one ("else") are listed by value.

    python tests/option_probe.py --lib PATH/libmlimgsynth_amd.so --out tests/golden/option_matrix.json

records the fixture.  It is recorded from the library of the commit BEFORE a change of the option code, never from the code under test."""
import ctypes as C
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlis_ffi as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INTS = [0, 1, 2, 3, 4, 5, -1, -2, 7, 8, 16, 31, 32, 33, 40, 256, 257, 512, 513, 1000, 1001, 8192, 8200, 65535, 65536]
FRACTIONS = [0.5, 0.99, 1.0, 1.5, 2.5, 4.5, 20, 20.5, 64, 64.5, 255, 32767, 32768]
MALFORMED = ["nan", "inf", "12x", "1e", " 1", "+1", '"1"', "1,2"]
BOOL_WORDS = ["yes", "no", "y", "n", "Y", "true", "false", "True", "maybe"]
ENUM_NAMES = ["none", "x", "y", "xy", "nearest", "bilinear", "bicubic", "box", "lanczos", "canny", "invert", "whole", "masked",
              "auto", "eps", "v", "off", "on"]
OTHER_NAMES = ["euler", "euler_a", "heun_a", "rk4", "rk4_a", "karras", "uniform", "f16", "bf16", "f32", "q8_0", "sd1", "sdxl", "tiny", "tinyv"]
PROMPTS = ["a (dog:1.5), with commas", "unbalanced )", "<lora:nosuch:0.5> x"]


def _uniq(seq):
    out = []
    for x in seq:
        if x not in out:
            out.append(x)
    return out


STR_VALUES = _uniq([""] + [str(i) for i in INTS] + [repr(f) if isinstance(f, float) else str(f) for f in FRACTIONS] + MALFORMED + BOOL_WORDS
                   + ENUM_NAMES + [n.upper() for n in ENUM_NAMES] + [n.replace("_", "-") for n in OTHER_NAMES if "_" in n] + OTHER_NAMES + PROMPTS)
VA_INTS = _uniq(INTS + [int(f) for f in FRACTIONS if float(f).is_integer()])
VA_DOUBLES = _uniq([float(i) for i in INTS] + [float(f) for f in FRACTIONS]) + [float("nan"), float("inf")]
VA_STRS = ["", "0", "1", "1,2", '"1"', " 1", "synth:tiny"] + PROMPTS
VA_VALUES = {"int": VA_INTS, "double": VA_DOUBLES, "uint64": VA_INTS, "str": VA_STRS}


def header_options():
    """{name: id} of the MLIS_Option enumerators of include/mlis_abi.h but MLIS_OPT__LAST; "cfg_scale" for MLIS_OPT_CFG_SCALE, "tiling" for MLIS_OPT_AMD_TILING"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlis_abi.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+enum\s+\w*\s*\{([^}]*)\}\s*MLIS_Option\s*;", hdr).group(1)
    opts = {}
    for name, val in re.findall(r"MLIS_OPT_(\w+)\s*=\s*(\d+)", body):
        if name != "_LAST":
            opts[(name[4:] if name.startswith("AMD_") else name).lower()] = int(val)
    return opts


def _va_arg(kind, v):
    if kind == "int":
        return C.c_int(v)
    if kind == "double":
        return C.c_double(v)
    if kind == "uint64":
        return C.c_uint64(v & 0xFFFFFFFFFFFFFFFF)
    return C.c_char_p(v.encode())


def _quote(err, text):
    """err with "{}" for the first place it quotes the value: after a ' ('V', 'V.safetensors') if there is one, else anywhere ("weight type V is ...")"""
    at = err.find("'" + text) + 1 or err.find(text) if text else err.find("''") + 1
    return err if at < 0 or (not text and at == 0) else err[:at] + "{}" + err[at + len(text):]


class _Probe:
    """one fresh context with a counting error handler; `first` is what the getter gives for option `oid` before anything is set"""

    def __init__(self, lib, kind, oid):
        self.lib, self.kind, self.oid, self.calls = lib, kind, oid, [0]
        self.m = F.Mlis(lib)
        self.handler = F.ERRHANDLER(lambda ud, ctx, ei: self.calls.__setitem__(0, self.calls[0] + 1))
        assert lib.mlis_option_set(self.m.ctx, F.OPT["ERROR_HANDLER"], self.handler, None) == 1
        self.first = self.got = self.get()
        self.err = self.m.err()
        self.calls[0] = 0

    def close(self):
        self.m.close()

    def get(self):
        """[return code, value]: the value as the option's kind says, None where mlis_option_get refused or wrote nothing"""
        buf = (C.c_ubyte * 16)(*([0xAA] * 16))
        rc = self.lib.mlis_option_get(self.m.ctx, self.oid, C.byref(buf))
        raw = bytes(buf)
        if rc != 1 or raw == b"\xaa" * 16:
            return [rc, None]
        assert raw[8:] == b"\xaa" * 8, "mlis_option_get wrote more than a pointer"
        if self.kind == "str":
            return [rc, C.cast(C.c_void_p(int.from_bytes(raw[:8], sys.byteorder)), C.c_char_p).value.decode()]
        assert raw[4:8] == b"\xaa" * 4, "mlis_option_get wrote more than 4 bytes for a number"
        if self.kind == "double":
            return [rc, "f32:%08x" % int.from_bytes(raw[:4], sys.byteorder)]
        return [rc, int.from_bytes(raw[:4], sys.byteorder, signed=True)]

    def outcome(self, text, rc):
        """of the set call that returned rc for the value written `text`"""
        err, n = self.m.err(), self.calls[0]       # (before the getter: where it refuses, it writes the error text itself)
        got = self.get()
        val = got[1]
        out = [rc, None if err == self.err else _quote(err, text), n, got[0],
               "{}" if str(val) == text and val is not None else "=" if got == self.got else val]
        self.got, self.err, self.calls[0] = got, self.m.err(), 0
        return out


def _fold(first, pairs):
    """{"first": .., "else": the most frequent outcome, "values": {value: outcome, where it is another}}"""
    keys = [json.dumps(o) for _, o in pairs]
    common = max(sorted(set(keys)), key=keys.count)
    return {"first": first, "else": json.loads(common), "values": {v: o for (v, o), k in zip(pairs, keys) if k != common}}


def probe(lib_path, arg_kind):
    """arg_kind: {option name: "int" | "double" | "uint64" | "str" | anything else = string form only}"""
    lib = F.bind(lib_path)
    opts = header_options()
    out = {"set_str": {}, "set": {}, "get_rc": {}, "set_unknown": []}
    for name, oid in sorted(opts.items(), key=lambda kv: kv[1]):
        kind = arg_kind[name]
        p = _Probe(lib, kind, oid)
        out["set_str"][name] = _fold(p.first, [(v, p.outcome(v, lib.mlis_option_set_str(p.m.ctx, name.encode(), v.encode()))) for v in STR_VALUES])
        p.close()
        if kind in VA_VALUES:
            p = _Probe(lib, kind, oid)
            out["set"][name] = _fold(p.first, [(repr(v), p.outcome(v if kind == "str" else repr(v), lib.mlis_option_set(p.m.ctx, oid, _va_arg(kind, v))))
                                               for v in VA_VALUES[kind]])
            p.close()
    p = _Probe(lib, "int", 0)
    for oid in range(256):
        out["get_rc"].setdefault(str(lib.mlis_option_get(p.m.ctx, oid, C.byref((C.c_ubyte * 16)()))), []).append(oid)
        if oid == 0 or oid not in opts.values():
            seen = [lib.mlis_option_set(p.m.ctx, oid, C.c_int(0)), p.m.err().replace(str(oid), "{}")]
            if seen not in out["set_unknown"]:
                out["set_unknown"].append(seen)
    p.close()
    return out


def dump(result, path):
    """one line per option and form"""
    with open(path, "w") as f:
        f.write("{\n")
        for part in ("set_str", "set"):
            rows = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"), allow_nan=False)) for k, v in result[part].items())
            f.write(' "%s": {\n%s\n },\n' % (part, rows))
        f.write(' "get_rc": %s,\n "set_unknown": %s\n}\n' % (json.dumps(result["get_rc"], separators=(",", ":")), json.dumps(result["set_unknown"])))


def main():
    import argparse
    from test_option_table_cpu import ARG_KIND
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the library to probe")
    ap.add_argument("--out", required=True, help="the JSON file to write")
    a = ap.parse_args()
    dump(probe(os.path.abspath(a.lib), ARG_KIND), a.out)


if __name__ == "__main__":
    main()
