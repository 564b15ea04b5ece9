"""Message classes for the All / Samples part of ReadServer's wire schema (src/service/readserver.proto:16-29,39-54):
ReadInfo, ResultAll, ReplyAll and Reply with its field `a`, re-typed as a FileDescriptorProto the way tests/proto_schema.py
re-types the rest, so the Python protobuf runtime can serialise and parse the bytes rsbwt_proto_encode_all_reply writes.
TEST INFRASTRUCTURE."""
from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

_F = descriptor_pb2.FieldDescriptorProto


def _field(msg, name, number, ftype, label, type_name=None):
    f = msg.field.add()
    f.name, f.number, f.type, f.label = name, number, ftype, label
    if type_name:
        f.type_name = type_name
    return f


def build():
    """(Reply, ResultAll, ReadInfo) message classes"""
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name = "readserver_all.proto"
    fd.syntax = "proto2"
    info = fd.message_type.add()
    info.name = "ReadInfo"  # readserver.proto:16-20
    _field(info, "g", 1, _F.TYPE_STRING, _F.LABEL_REQUIRED)
    _field(info, "c", 2, _F.TYPE_INT32, _F.LABEL_REQUIRED)
    _field(info, "l", 3, _F.TYPE_INT32, _F.LABEL_REQUIRED)
    ra = fd.message_type.add()
    ra.name = "ResultAll"  # :26-29
    _field(ra, "r", 1, _F.TYPE_STRING, _F.LABEL_REQUIRED)
    _field(ra, "s", 2, _F.TYPE_MESSAGE, _F.LABEL_REPEATED, ".ReadInfo")
    rall = fd.message_type.add()
    rall.name = "ReplyAll"  # :51-54
    _field(rall, "forward_matches", 1, _F.TYPE_MESSAGE, _F.LABEL_REPEATED, ".ResultAll")
    _field(rall, "revcomp_matches", 2, _F.TYPE_MESSAGE, _F.LABEL_REPEATED, ".ResultAll")
    rr = fd.message_type.add()
    rr.name = "ResultReads"  # :35-37
    _field(rr, "r", 1, _F.TYPE_STRING, _F.LABEL_REQUIRED)
    rreads = fd.message_type.add()
    rreads.name = "ReplyReads"  # :61-64
    _field(rreads, "forward_matches", 1, _F.TYPE_MESSAGE, _F.LABEL_REPEATED, ".ResultReads")
    _field(rreads, "revcomp_matches", 2, _F.TYPE_MESSAGE, _F.LABEL_REPEATED, ".ResultReads")
    rep = fd.message_type.add()
    rep.name = "Reply"  # :39-49 (c and s, which these replies never carry, are left out)
    e = rep.enum_type.add()
    e.name = "RequestType"
    for n, v in (("CountReads", 1), ("ExactMatch", 2), ("KmerMatch", 3), ("SiteMatch", 4)):
        x = e.value.add(); x.name, x.number = n, v
    e = rep.enum_type.add()
    e.name = "ReplyType"
    for n, v in (("ReplyCount", 1), ("ReplyReads", 2), ("ReplyAll", 3), ("ResultSamples", 4)):
        x = e.value.add(); x.name, x.number = n, v
    _field(rep, "rt", 1, _F.TYPE_ENUM, _F.LABEL_REQUIRED, ".Reply.RequestType")
    _field(rep, "t", 2, _F.TYPE_ENUM, _F.LABEL_REQUIRED, ".Reply.ReplyType")
    _field(rep, "q", 3, _F.TYPE_STRING, _F.LABEL_REQUIRED)
    _field(rep, "r", 5, _F.TYPE_MESSAGE, _F.LABEL_OPTIONAL, ".ReplyReads")
    _field(rep, "a", 6, _F.TYPE_MESSAGE, _F.LABEL_OPTIONAL, ".ReplyAll")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = lambda n: message_factory.GetMessageClass(pool.FindMessageTypeByName(n))  # noqa: E731
    return get("Reply"), get("ResultAll"), get("ReadInfo")


def records(value, hash_map, size_of_sample, has_other):
    """value -> [(g, c, l)] as src/service/service.cpp:1332-1347 spells them, cut at the last whole record"""
    rec = size_of_sample + (2 if has_other else 0)
    out = []
    for pos in range(0, len(value) - rec + 1, rec) if rec else ():
        g = hash_map.get(value[pos:pos + size_of_sample], "")
        sc = lambda b: (b - 256 if b > 127 else b) - 33  # noqa: E731  (int)(signed char) - 33
        out.append((g, sc(value[pos + size_of_sample]), sc(value[pos + size_of_sample + 1])) if has_other else (g, 0, 0))
    return out


def all_reply(Reply, request_type, return_type, q, revcomp, reads, values, hash_map, size_of_sample, has_other):
    """the Reply QueryTask::run / KmerTask::run send for All and Samples, serialised by the protobuf runtime"""
    r = Reply()
    r.rt, r.t, r.q = request_type, return_type, q
    r.a.SetInParent()  # mutable_a(): present even when empty
    for read, value in zip(reads, values):
        m = (r.a.revcomp_matches if revcomp else r.a.forward_matches).add()
        m.r = read
        for g, c, l in records(value, hash_map, size_of_sample, has_other):
            s = m.s.add()
            s.g, s.c, s.l = g, c, l
    return r.SerializeToString()
