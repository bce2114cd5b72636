"""The tests' own reading of include/phendiff_hip.h.  It shares no code with the package's reader (phendiff_amd/_abi.py): what the
binding derives from the header is held against this second reading of the same text, and against the literals the tests freeze."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phendiff_hip.h")


def source():
    with open(HEADER) as f:
        return f.read()


def struct_names():
    """Every pd_* a ``typedef struct { ... } pd_*;`` of the header names, in its order."""
    return re.findall(r"typedef struct(?:\s+\w+)?\s*\{[^{}]*\}\s*(pd_\w+)\s*;", source(), flags=re.S)


def header_fields(cname):
    """The field names of one struct of the header, in declaration order (comma lists expanded)."""
    body = re.search(r"typedef struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*" + cname + ";", source(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?$", part.strip())[0])
    return fields


def define(name):
    """The integer a ``#define`` of the header gives ``name``."""
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", source()).group(1))


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", source(), flags=re.S)
    return sorted(set(re.findall(r"\b(pd_[a-z0-9_]+)\s*\(", src)))
