"""Handler configuration with the reference's validation and error texts.

Mirrors what StreamMetricsHandler::start does before any packet flows
(src/StreamHandler.h:94-152) for the two handlers on the path:

  * validate_configs: every key of the handler config must be one of the handler's
    _config_defs, a window config key, "enable" or "disable"
    (NetStreamHandler.h:204-209, DnsStreamHandler.h:381-397);
  * process_groups: the handler's default groups, then "disable", then "enable", each
    list stopping at "all" (src/StreamHandler.h:111-133; defaults
    NetStreamHandler.cpp:53-56, DnsStreamHandler.cpp:52-57);
  * the DNS filters and configs (DnsStreamHandler::start, :60-201).

The result is the typed pv_config / pv_dns_filters content the C-ABI takes; the GPU
path never sees a config it does not implement (unbuilt keys raise, never ignored).
"""
from __future__ import annotations


class PvError(RuntimeError):
    """Base of every error pktvisor_amd raises."""


class StreamHandlerException(PvError):
    """visor::StreamHandlerException (src/StreamHandler.h)"""


class ConfigException(PvError):
    """visor::ConfigException (src/Configurable.h)"""


WINDOW_CONFIG_DEFS = ("deep_sample_rate", "num_periods", "topn_count", "topn_percentile_threshold")
NET_CONFIG_DEFS = ("geoloc_notfound", "asn_notfound", "only_geoloc_prefix", "only_asn_number", "recorded_stream")
DNS_CONFIG_DEFS = ("exclude_noerror", "only_rcode", "only_queries", "only_responses", "only_dnssec_response",
                   "answer_count", "only_qtype", "only_qname", "only_qname_suffix", "geoloc_notfound", "asn_notfound",
                   "dnstap_msg_type", "public_suffix_list", "recorded_stream", "xact_ttl_secs", "xact_ttl_ms")
# group name -> pv_net_group / pv_dns_group bit (include/pvgpu.h); listed sorted, as std::map iterates
NET_GROUP_DEFS = {"cardinality": 1 << 1, "counters": 1 << 0, "top_geo": 1 << 2, "top_ips": 1 << 3}
DNS_GROUP_DEFS = {"cardinality": 1 << 0, "counters": 1 << 1, "dns_transaction": 1 << 4, "histograms": 1 << 3,
                  "quantiles": 1 << 2, "top_ecs": 1 << 5, "top_ports": 1 << 8, "top_qnames": 1 << 6,
                  "top_qnames_details": 1 << 7}
NET_DEFAULT_GROUPS = ("counters", "cardinality", "top_geo", "top_ips")
DNS_DEFAULT_GROUPS = ("cardinality", "counters", "quantiles", "dns_transaction", "top_qnames", "top_ports")
DNSTAP_MSG_TYPES = ("auth", "client", "forwarder", "resolver", "stub", "tool", "update")
# dnstap Message.Type numbers of each dnstap_msg_type (DnsStreamHandler.h:340-347; dnstap.proto:160-227)
DNSTAP_TYPE_PAIRS = {"auth": (1, 2), "resolver": (3, 4), "client": (5, 6), "forwarder": (7, 8), "stub": (9, 10),
                     "tool": (11, 12), "update": (13, 14)}
GROUPS_SET = 0x80000000  # PV_GROUPS_SET


def validate_configs(cfg: dict, defs) -> None:
    """StreamMetricsHandler::validate_configs (src/StreamHandler.h:135-152)"""
    for key in cfg:
        if key in WINDOW_CONFIG_DEFS or key in defs or key in ("enable", "disable", "_internal_tap_name"):
            continue
        raise StreamHandlerException(f"{key} is an invalid/unsupported config or filter. The valid configs/filters are: "
                                     f"{', '.join(defs)}, {', '.join(WINDOW_CONFIG_DEFS)}")


def _string_list(cfg: dict, key: str) -> list:
    v = cfg[key]
    if not isinstance(v, (list, tuple)) or not all(isinstance(x, str) for x in v):
        raise ConfigException(f"wrong type for key: {key}")  # Configurable::config_get (src/Configurable.h:110)
    return list(v)


def process_groups(cfg: dict, group_defs: dict, defaults) -> int:
    """StreamMetricsHandler::process_groups (src/StreamHandler.h:94-133): the enabled group bits"""
    bits = 0
    for g in defaults:
        bits |= group_defs[g]

    def one(g):
        if g not in group_defs:
            raise StreamHandlerException(f"{g} is an invalid/unsupported metric group. The valid groups are: all, "
                                         + ", ".join(sorted(group_defs)))
        return group_defs[g]

    if "disable" in cfg:
        for g in _string_list(cfg, "disable"):
            if g == "all":
                bits = 0
                break
            bits &= ~one(g)
    if "enable" in cfg:
        for g in _string_list(cfg, "enable"):
            if g == "all":
                for v in group_defs.values():
                    bits |= v
                break
            bits |= one(g)
    return bits


def _bool(cfg: dict, key: str) -> bool:
    v = cfg.get(key, False)
    if not isinstance(v, bool):
        raise ConfigException(f"wrong type for key: {key}")
    return v


def _uint(cfg: dict, key: str) -> int:
    v = cfg[key]
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ConfigException(f"wrong type for key: {key}")
    return v


def window_config(cfgs) -> dict:
    """The window config keys (AbstractMetricsManager::AbstractMetricsManager,
    src/AbstractMetricsManager.h:351-389): num_periods 1..10, deep_sample_rate 1..100, topn_count,
    topn_percentile_threshold 0..99 — one value shared by both handlers here."""
    out = {}
    for cfg in cfgs:
        for k in WINDOW_CONFIG_DEFS:
            if k in cfg:
                v = _uint(cfg, k)
                if k in out and out[k] != v:
                    raise ConfigException(f"{k} differs between the net and dns handler configs")
                out[k] = v
    np = out.get("num_periods", 5)
    if not 1 <= np <= 10:
        raise ConfigException("num_periods must be between 1 and 10")
    if "deep_sample_rate" in out:
        # clamped, not refused (AbstractMetricsManager.h:357-365)
        out["deep_sample_rate"] = max(1, min(100, out["deep_sample_rate"]))
    if out.get("topn_percentile_threshold", 0) > 99:
        raise ConfigException("topn_percentile_threshold must be between 0 and 99")
    return out


def net_start(cfg: dict, geo_enabled=None) -> dict:
    """NetStreamHandler::start (src/handlers/net/v1/NetStreamHandler.cpp:45-130) up to the
    signal wiring: {"groups": bits | GROUPS_SET, "filter_all": bool}.

    geo_enabled = (city database enabled, ASN database enabled), the reference's
    HandlerModulePlugin::city / asn: the geo filters then come back typed under "filters"
    (the pv_net_filters fields), and "filter_all" is set only where a configured filter family has
    no database (_filtering :223-283: !enabled() => will_filter). Without the keyword no database
    is enabled and the result is what it always was."""
    validate_configs(cfg, NET_CONFIG_DEFS)
    groups = process_groups(cfg, NET_GROUP_DEFS, NET_DEFAULT_GROUPS)
    out = {"groups": groups | GROUPS_SET, "filter_all": False}
    filters = {"geoloc_notfound": False, "asn_notfound": False, "only_geoloc_prefix": None, "only_asn_number": None}
    # the geo / ASN filters match a MaxMind lookup; with no database enabled every packet is
    # filtered (_filtering :223-283: !city->enabled() => will_filter)
    city_on, asn_on = (bool(geo_enabled[0]), bool(geo_enabled[1])) if geo_enabled is not None else (False, False)
    if _bool(cfg, "geoloc_notfound"):
        filters["geoloc_notfound"] = True
    if _bool(cfg, "asn_notfound"):
        filters["asn_notfound"] = True
    if "only_geoloc_prefix" in cfg:
        filters["only_geoloc_prefix"] = list(_string_list(cfg, "only_geoloc_prefix"))
    if "only_asn_number" in cfg:
        numbers = list(_string_list(cfg, "only_asn_number"))
        for number in numbers:
            if not number.isdigit():
                raise ConfigException(f"NetStreamHandler: only_asn_number filter contained an invalid/unsupported value: {number}")
        filters["only_asn_number"] = numbers
    geoloc = filters["geoloc_notfound"] or filters["only_geoloc_prefix"] is not None
    asn = filters["asn_notfound"] or filters["only_asn_number"] is not None
    if (geoloc and not city_on) or (asn and not asn_on):
        out["filter_all"] = True
    if geo_enabled is not None and (geoloc or asn):
        out["filters"] = filters
    return out


DHCP_CONFIG_DEFS = ("recorded_stream", "xact_ttl_secs", "xact_ttl_ms")


def dhcp_start(cfg: dict) -> dict:
    """DhcpStreamHandler::start (src/handlers/dhcp/DhcpStreamHandler.cpp:41-69) up to the signal
    wiring: {"recorded_stream": bool, "xact_ttl_ms": int (0: the TransactionManager's 5000)}.
    The handler has no metric groups and no filters; xact_ttl_ms wins over xact_ttl_secs."""
    validate_configs(cfg, DHCP_CONFIG_DEFS)
    ttl = 0
    if "xact_ttl_ms" in cfg:
        ttl = _uint(cfg, "xact_ttl_ms")
    elif "xact_ttl_secs" in cfg:
        ttl = _uint(cfg, "xact_ttl_secs") * 1000
    if ttl > 0xFFFFFFFF:
        raise ConfigException("wrong type for key: xact_ttl_ms")
    return {"recorded_stream": "recorded_stream" in cfg, "xact_ttl_ms": ttl}


BGP_CONFIG_DEFS = ("recorded_stream",)


def bgp_start(cfg: dict) -> dict:
    """BgpStreamHandler::start (src/handlers/bgp/BgpStreamHandler.cpp:21-43) up to the signal
    wiring: {"recorded_stream": bool}. The handler has no metric groups and no filters."""
    validate_configs(cfg, BGP_CONFIG_DEFS)
    return {"recorded_stream": "recorded_stream" in cfg}


# the flow handler (src/handlers/flow/FlowStreamHandler.h:384-412; defaults FlowStreamHandler.cpp:95-101);
# "ports" is this package's own key: the UDP destination ports of the flow input
FLOW_CONFIG_DEFS = ("device_map", "enrichment", "only_device_interfaces", "only_ips", "only_ports", "only_directions",
                    "geoloc_notfound", "asn_notfound", "summarize_ips_by_asn", "subnets_for_summarization",
                    "exclude_asns_from_summarization", "exclude_unknown_asns_from_summarization",
                    "exclude_ips_from_summarization", "sample_rate_scaling", "recorded_stream")
FLOW_OWN_CONFIG_DEFS = ("ports",)
# group name -> pv_flow_group bit (include/pvgpu.h)
FLOW_GROUP_DEFS = {"by_bytes": 1 << 5, "by_packets": 1 << 6, "cardinality": 1 << 1, "conversations": 1 << 7,
                   "counters": 1 << 0, "top_geo": 1 << 9, "top_interfaces": 1 << 10, "top_ips": 1 << 2,
                   "top_ips_ports": 1 << 4, "top_ports": 1 << 3, "top_tos": 1 << 8}
FLOW_DEFAULT_GROUPS = ("counters", "cardinality", "top_ips", "top_ports", "top_ips_ports", "by_bytes", "by_packets")
FLOW_NOT_BUILT = ("device_map", "enrichment", "only_device_interfaces", "only_ips", "only_ports", "only_directions",
                  "geoloc_notfound", "asn_notfound", "summarize_ips_by_asn", "subnets_for_summarization",
                  "exclude_asns_from_summarization", "exclude_unknown_asns_from_summarization",
                  "exclude_ips_from_summarization")
FLOW_MAX_PORTS = 8


def flow_start(cfg: dict) -> dict:
    """FlowStreamHandler::start (src/handlers/flow/FlowStreamHandler.cpp:86-269) up to the signal
    wiring: {"groups": bits | GROUPS_SET, "recorded_stream": bool, "ports": [int]}. The filters,
    enrichment and summarization are not built: their keys raise. sample_rate_scaling is sFlow's
    (:352) and has no effect on NetFlow."""
    cfg = dict(cfg)
    ports = cfg.pop("ports", [])
    validate_configs(cfg, FLOW_CONFIG_DEFS)
    groups = process_groups(cfg, FLOW_GROUP_DEFS, FLOW_DEFAULT_GROUPS)
    for k in FLOW_NOT_BUILT:
        if k in cfg:
            raise ConfigException(f"{k} is not supported by the GPU flow handler")
    if "sample_rate_scaling" in cfg:
        _bool(cfg, "sample_rate_scaling")
    if not isinstance(ports, (list, tuple)) or not all(isinstance(p, int) and not isinstance(p, bool) and 0 <= p <= 65535
                                                       for p in ports):
        raise ConfigException("wrong type for key: ports")
    if len(ports) > FLOW_MAX_PORTS:
        raise ConfigException(f"ports: at most {FLOW_MAX_PORTS} UDP ports")
    return {"groups": groups | GROUPS_SET, "recorded_stream": "recorded_stream" in cfg, "ports": [int(p) for p in ports]}


def iana_port_rows(text: str) -> list:
    """IpPort::set_csv_iana_ports (src/IpPort.cpp:34-69) over the text of an IANA-style CSV: the rows
    (last, first, protocol number, name) in file order. The reference's reader splits at every comma
    (no quoting), trims blanks and tabs, and wants as many columns in a row as the header has; a row
    that fails (a column count, a port that is no number) is dropped together with the line after
    it (the handler's in.next_line())."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if not lines:
        return []

    def cols(line):
        return [c.strip(" \t") for c in line.rstrip("\r").split(",")]

    header = cols(lines[0])
    try:
        want = [header.index(n) for n in ("Service Name", "Port Number", "Transport Protocol")]
    except ValueError:
        raise ConfigException("flow_port_csv: missing a column of Service Name, Port Number, Transport Protocol")

    def number(txt):
        # std::stoul: leading blanks, an optional sign, then digits; what follows is ignored
        t = txt.lstrip(" \t\n\v\f\r")
        neg = t[:1] == "-"
        if t[:1] in "+-":
            t = t[1:]
        k = 0
        while k < len(t) and t[k].isdigit() and t[k].isascii():
            k += 1
        if k == 0:
            raise ValueError(txt)
        v = int(t[:k])
        if v >= 1 << 64:
            raise ValueError(txt)
        return ((-v if neg else v) & 0xFFFFFFFFFFFFFFFF) & 0xFFFF

    rows = []
    i = 1
    while i < len(lines):
        c = cols(lines[i])
        i += 1
        try:
            if len(c) != len(header):
                raise ValueError("columns")
            service, ports, proto = (c[k] for k in want)
            if not service or not ports or proto not in ("tcp", "udp"):
                continue
            cut = ports.find("-")
            if cut >= 0:
                first, last = number(ports[:cut]), number(ports[cut + 1:])
            else:
                first = last = number(ports)
            rows.append((last, first, 6 if proto == "tcp" else 17, service))
        except ValueError:
            i += 1  # the handler's in.next_line(): the line after a bad row goes too
    return rows


# Net v2 (src/handlers/net/v2/NetStreamHandler.h:25-31,262-267; defaults :47-52)
NET2_GROUP_DEFS = {"cardinality": 1 << 1, "counters": 1 << 0, "quantiles": 1 << 2, "top_geo": 1 << 3, "top_ips": 1 << 4}
NET2_DEFAULT_GROUPS = ("counters", "cardinality", "quantiles", "top_geo", "top_ips")


def net2_start(cfg: dict, geo: bool = False):
    """NetStreamHandler v2 start (src/handlers/net/v2/NetStreamHandler.cpp:45-95) up to the
    signal wiring: the enabled group bits | GROUPS_SET. Its geo / ASN filters need a MaxMind
    database and the v2 geo switch (pv_set_v2_geo): without geo=True they raise.

    geo=True: {"groups": bits | GROUPS_SET, "filters": the pv_net_filters fields or None}, the four
    keys typed as net_start types them for v1 (:61-88); pv_set_net2_filters decides, family by
    family, against the attached databases."""
    validate_configs(cfg, NET_CONFIG_DEFS)
    groups = process_groups(cfg, NET2_GROUP_DEFS, NET2_DEFAULT_GROUPS)
    if not geo:
        for k in ("geoloc_notfound", "asn_notfound", "only_geoloc_prefix", "only_asn_number"):
            if k in cfg:
                raise ConfigException(f"{k} is not supported by the GPU Net v2 handler")
        return groups | GROUPS_SET
    filters = {"geoloc_notfound": _bool(cfg, "geoloc_notfound"), "asn_notfound": _bool(cfg, "asn_notfound"),
               "only_geoloc_prefix": None, "only_asn_number": None}
    if "only_geoloc_prefix" in cfg:
        filters["only_geoloc_prefix"] = list(_string_list(cfg, "only_geoloc_prefix"))
    if "only_asn_number" in cfg:
        numbers = list(_string_list(cfg, "only_asn_number"))
        for number in numbers:
            if not number.isdigit():
                raise ConfigException(f"NetStreamHandler: only_asn_number filter contained an invalid/unsupported value: {number}")
        filters["only_asn_number"] = numbers
    on = filters["geoloc_notfound"] or filters["asn_notfound"] or filters["only_geoloc_prefix"] is not None \
        or filters["only_asn_number"] is not None
    return {"groups": groups | GROUPS_SET, "filters": filters if on else None}


# DNS v2 (src/handlers/dns/v2/DnsStreamHandler.h:40-52,549-575; defaults .cpp:51-57)
DNS2_GROUP_DEFS = {"cardinality": 1 << 0, "counters": 1 << 1, "quantiles": 1 << 2, "top_ecs": 1 << 3,
                   "top_qtypes": 1 << 4, "top_rcodes": 1 << 5, "top_size": 1 << 6, "top_qnames": 1 << 7,
                   "top_ports": 1 << 8, "xact_times": 1 << 9}
DNS2_DEFAULT_GROUPS = ("cardinality", "counters", "quantiles", "top_qnames", "top_rcodes", "top_qtypes")
DNS2_CONFIG_DEFS = ("exclude_noerror", "only_rcode", "only_dnssec_response", "only_xact_directions", "answer_count",
                    "only_qtype", "only_qname", "only_qname_suffix", "geoloc_notfound", "asn_notfound", "dnstap_msg_type",
                    "public_suffix_list", "recorded_stream", "xact_ttl_secs", "xact_ttl_ms")
DNS2_FILTER_KEYS = ("exclude_noerror", "only_rcode", "only_dnssec_response", "answer_count", "only_qtype", "only_qname",
                    "only_qname_suffix")


def dns2_start(cfg: dict, geo: bool = False) -> dict:
    """DnsStreamHandler v2 start (src/handlers/dns/v2/DnsStreamHandler.cpp:43-236) up to the
    signal wiring: {"groups": bits | GROUPS_SET, "filters": pv_dns_filters fields (v2) or None,
    "xact_ttl_ms": int|None}. The geo / ASN filters (no MaxMind database) are not built for the
    GPU v2 handler; top_ecs keeps
    its geo / ASN tops empty (no MaxMind database).

    geo=True (the v2 geo switch, pv_set_v2_geo): geoloc_notfound / asn_notfound do not raise and
    come back typed under "v2_geo" (the pv_v2_geo dns_* fields): query-branch filters matched on the
    device against the attached databases (dns/v2/DnsStreamHandler.cpp:551-574)."""
    from pktvisor_amd import dns_filter_config
    validate_configs(cfg, DNS2_CONFIG_DEFS)
    groups = process_groups(cfg, DNS2_GROUP_DEFS, DNS2_DEFAULT_GROUPS)
    for k in ("geoloc_notfound", "asn_notfound"):
        if k in cfg and not geo:
            raise ConfigException(f"{k} is not supported by the GPU DNS v2 handler")
    # dnstap_msg_type (dns/v2/DnsStreamHandler.cpp:176-190): as v1's
    if "dnstap_msg_type" in cfg and cfg["dnstap_msg_type"] not in DNSTAP_MSG_TYPES:
        raise ConfigException("DnsStreamHandler: dnstap_msg_type contained an invalid/unsupported type. Valid types: "
                              + ", ".join(DNSTAP_MSG_TYPES))
    mask = 0
    if "dnstap_msg_type" in cfg:
        q, r = DNSTAP_TYPE_PAIRS[cfg["dnstap_msg_type"]]
        mask = (1 << q) | (1 << r)
    filters = None
    psl = _bool(cfg, "public_suffix_list")  # _configs (dns/v2/DnsStreamHandler.cpp:192-194,612-619)
    if any(k in cfg for k in DNS2_FILTER_KEYS) or "only_xact_directions" in cfg or psl:
        filters = dns_filter_config({k: cfg[k] for k in DNS2_FILTER_KEYS if k in cfg}, v2=True)
        filters["v2"] = 1
        filters["public_suffix_list"] = 1 if psl else 0
        # only_xact_directions (:107-122): every direction filtered but the listed ones
        if "only_xact_directions" in cfg:
            dis = 7
            for d in _string_list(cfg, "only_xact_directions"):
                if d not in ("in", "out", "unknown"):
                    raise ConfigException("DnsStreamHandler: only_xact_directions filter contained an invalid/unsupported "
                                          f"direction: {d}")
                dis &= ~{"in": 1, "out": 2, "unknown": 4}[d]
            filters["xact_dirs_disabled"] = dis
    ttl = None
    if "xact_ttl_ms" in cfg:
        ttl = _uint(cfg, "xact_ttl_ms")
    elif "xact_ttl_secs" in cfg:
        ttl = _uint(cfg, "xact_ttl_secs") * 1000
    out = {"groups": groups | GROUPS_SET, "filters": filters, "xact_ttl_ms": ttl, "dnstap_mask": mask}
    if geo:
        out["v2_geo"] = {"geoloc_notfound": _bool(cfg, "geoloc_notfound"), "asn_notfound": _bool(cfg, "asn_notfound")}
    return out


def dns_start(cfg: dict, dns_geo: bool = False) -> dict:
    """DnsStreamHandler::start (src/handlers/dns/v1/DnsStreamHandler.cpp:43-201) up to the signal
    wiring: {"groups": bits | GROUPS_SET, "filters": pv_dns_filters fields, "xact_ttl_ms": int|None}.
    dns_geo: the handler reads the attached GeoIP databases (pv_set_dns_geo); geoloc_notfound /
    asn_notfound are then typed, under "dns_geo" (the pv_dns_geo fields), instead of filter_all."""
    from pktvisor_amd import dns_filter_config
    validate_configs(cfg, DNS_CONFIG_DEFS)
    groups = process_groups(cfg, DNS_GROUP_DEFS, DNS_DEFAULT_GROUPS)
    fkeys = ("exclude_noerror", "only_rcode", "answer_count", "only_queries", "only_responses", "only_qtype",
             "only_qname", "only_qname_suffix", "only_dnssec_response")
    filters = dns_filter_config({k: cfg[k] for k in fkeys if k in cfg})
    # with no geo database enabled, geoloc_notfound / asn_notfound filter every packet (:619-642)
    filters["filter_all"] = 1 if (_bool(cfg, "geoloc_notfound") or _bool(cfg, "asn_notfound")) else 0
    geo = None
    if dns_geo:
        # matched on the device against the attached databases; a family whose database is not
        # attached filters every message there (the reference's !enabled() branch)
        geo = {"enable": 1, "geoloc_notfound": 1 if _bool(cfg, "geoloc_notfound") else 0,
               "asn_notfound": 1 if _bool(cfg, "asn_notfound") else 0}
        filters["filter_all"] = 0
    if "dnstap_msg_type" in cfg and cfg["dnstap_msg_type"] not in DNSTAP_MSG_TYPES:
        raise ConfigException("DnsStreamHandler: dnstap_msg_type contained an invalid/unsupported type. Valid types: "
                              + ", ".join(DNSTAP_MSG_TYPES))
    # public_suffix_list (_configs, dns/v1/DnsStreamHandler.cpp:187-189,648-657): a config the DNS
    # pass applies (pv_dns_filters.public_suffix_list)
    filters["public_suffix_list"] = 1 if _bool(cfg, "public_suffix_list") else 0
    ttl = None
    if "xact_ttl_ms" in cfg:
        ttl = _uint(cfg, "xact_ttl_ms")
    elif "xact_ttl_secs" in cfg:
        ttl = _uint(cfg, "xact_ttl_secs") * 1000
    mask = 0
    if "dnstap_msg_type" in cfg:
        q, r = DNSTAP_TYPE_PAIRS[cfg["dnstap_msg_type"]]
        mask = (1 << q) | (1 << r)
    out = {"groups": groups | GROUPS_SET, "filters": filters, "xact_ttl_ms": ttl, "dnstap_mask": mask}
    if geo is not None:
        out["dns_geo"] = geo
    return out
