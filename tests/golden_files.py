"""Stored test vectors under tests/golden/: the legacy TASO rule corpus
(graph_subst_3_v2 as protobuf and as gzipped JSON), the DLRM protobuf strategy
files, and the function names of the legacy flexflow_c.h surface."""
import gzip
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RULES_PB = os.path.join(GOLDEN, "substitutions", "graph_subst_3_v2.pb")
RULES_JSON_GZ = os.path.join(GOLDEN, "substitutions", "graph_subst_3_v2.json.gz")
DLRM_STRATEGIES = os.path.join(GOLDEN, "dlrm_strategies")
C_API_NAMES = os.path.join(GOLDEN, "flexflow_c_function_names.txt")


def rules_json_text() -> str:
    """The rule corpus as JSON text."""
    with gzip.open(RULES_JSON_GZ, "rt") as f:
        return f.read()


def rules_json_file(directory) -> str:
    """The rule corpus unpacked to ``directory``/graph_subst_3_v2.json (for the
    command-line tools, which take a path)."""
    path = os.path.join(str(directory), "graph_subst_3_v2.json")
    with open(path, "w") as f:
        f.write(rules_json_text())
    return path
