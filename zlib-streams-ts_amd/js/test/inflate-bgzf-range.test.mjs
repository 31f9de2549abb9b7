// BGZF ranges by virtual offset through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_inflate_batch_bgzf_range): decompressBatch*(inputs, "gzip", {members: "bgzf", ranges: [[vb, ve], ...]}) on a
// file of blocks built here around node's own raw deflate -- two ranges over the one file, with and without
// outCapacity, a range whose offsets follow no chain beside them -- and the rejection rules.
//   node inflate-bgzf-range.test.mjs cpu   -- the argument checks and bgzfRangeOutLength only (no GPU needed)
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;
const EOF = new Uint8Array(Buffer.from("1f8b08040000000000ff0600424302001b0003000000000000000000", "hex"));
const cat = (parts) => new Uint8Array(Buffer.concat(parts.map((p) => Buffer.from(p.buffer, p.byteOffset, p.length))));

function block(data) {
  const buf = Buffer.from(data.buffer, data.byteOffset, data.length);
  const raw = zlib.deflateRawSync(buf, { level: 6 });
  const gz = zlib.gzipSync(buf);
  const b = Buffer.alloc(18 + raw.length + 8);
  Buffer.from("1f8b08040000000000ff0600424302000000", "hex").copy(b, 0);
  b.writeUInt16LE(b.length - 1, 16);
  raw.copy(b, 18);
  gz.copy(b, 18 + raw.length, gz.length - 8, gz.length - 4);
  b.writeUInt32LE(data.length, b.length - 4);
  return new Uint8Array(b);
}
// the file and its blocks' starts in it, the end of the file last
function bgzf(x, size) {
  const parts = [], starts = [];
  let at = 0;
  for (let a = 0; a < x.length; a += size) {
    parts.push(block(x.subarray(a, Math.min(a + size, x.length))));
    starts.push(at);
    at += parts[parts.length - 1].length;
  }
  starts.push(at, at + EOF.length);  // the end-of-file block, the end
  return [cat([...parts, EOF]), starts];
}

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

const x = corpus.text(corpus.streamSeed(5), 1000);
const [file, starts] = bgzf(x, 300);  // blocks of 300, 300, 300 and 100 bytes
const v = api.virtualOffset;
// from byte 7 of block 0 to byte 11 of block 2; from byte 299 of block 1 to the end of the file
const ranges = [[v(starts[0], 7), v(starts[2], 11)], [v(starts[1], 299), v(starts[5])]];
const want = [x.subarray(7, 611), x.subarray(599, 1000)];

async function argumentChecks() {
  const type = (e) => e instanceof TypeError;
  expect(v(5, 3) === 327683n && v(5) === 327680n, "virtualOffset");
  await rejects(api.decompressBatch([file], "gzip", { outCapacity: 1000, ranges: [ranges[0]] }), type, "without members: a TypeError");
  await rejects(api.decompressBatch([file], "gzip", { outCapacity: 1000, members: true, ranges: [ranges[0]] }), type, "members: true: a TypeError");
  await rejects(api.decompressBatch([file, file], "gzip", { members: "bgzf", ranges: [ranges[0]] }), type, "one pair per input");
  await rejects(api.decompressBatch([file], "gzip", { members: "bgzf", ranges: [[7, 9]] }), type, "numbers are no virtual offsets");
  await rejects(api.decompressBatch([file], "gzip", { members: "bgzf", ranges: [[0n, -1n]] }), type, "a negative offset");
  // the sizing: host arithmetic over the headers
  expect(api.bgzfRangeOutLength(file, ...ranges[0]) === 604 && api.bgzfRangeOutLength(file, ...ranges[1]) === 401 &&
         api.bgzfRangeOutLength(file, 0n, v(file.length)) === 1000 && api.bgzfRangeOutLength(file, v(starts[2]), v(starts[2])) === 0,
         "bgzfRangeOutLength of ranges that follow the chain");
  expect(api.bgzfRangeOutLength(file, v(starts[1] + 3), v(starts[2])) === null && api.bgzfRangeOutLength(file, v(0, 301), v(starts[2])) === null &&
         api.bgzfRangeOutLength(file, v(starts[2]), v(starts[1])) === null && api.bgzfRangeOutLength(file, 0n, v(file.length + 1)) === null,
         "bgzfRangeOutLength of a start inside a block, a position above ISIZE, a begin behind the end, an end past the file");
  await rejects(api.decompressBatch([file, file], "gzip", { members: "bgzf", ranges: [ranges[0], [v(3), v(starts[1])]] }),
                (e) => type(e) && /input 1: the virtual offsets do not follow a chain of BGZF blocks: give outCapacity/.test(e.message),
                "without outCapacity, no chain: a TypeError");
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  // two ranges over the one file, sized from the headers
  const outs = await api.decompressBatch([file, file], "gzip", { members: "bgzf", ranges });
  expect(same(outs[0], want[0]) && same(outs[1], want[1]), "two ranges, no outCapacity");
  // with capacities, a range that follows no chain between them: it fails alone
  const d = await api.decompressBatchDetailed([file, file, file], "gzip",
                                              { members: "bgzf", outCapacity: [604, 64, 401], ranges: [ranges[0], [v(starts[1] + 3), v(starts[2])], ranges[1]] });
  expect(String(Array.from(d.status)) === "1,-3,1" && d.message[1] === "virtual offsets do not follow a chain of BGZF blocks" &&
         d.consumed[1] === starts[1] + 3 && d.outputs[1].length === 0, "the range that follows no chain");
  expect(same(d.outputs[0], want[0]) && same(d.outputs[2], want[1]) && d.consumed[0] === starts[3] && d.consumed[2] === file.length,
         "its neighbours, and consumed: behind the last decoded block");
  expect(d.check[0] === zlib.gzipSync(Buffer.from(want[0])).readUInt32LE(zlib.gzipSync(Buffer.from(want[0])).length - 8), "check: the crc32 of the delivered bytes");
  // an empty input in front of a different one: its empty range at offset 0 (ce == in_len) is legal, and the input
  // behind it is copied although both begin at the same offset of the job's buffer
  const e = await api.decompressBatchDetailed([new Uint8Array(0), file, file, new Uint8Array(0), file], "gzip",
                                              { members: "bgzf", ranges: [[0n, 0n], ranges[0], ranges[1], [0n, 0n], ranges[0]] });
  expect(String(Array.from(e.status)) === "1,1,1,1,1" && e.outputs[0].length === 0 && e.outputs[3].length === 0 &&
         same(e.outputs[1], want[0]) && same(e.outputs[2], want[1]) && same(e.outputs[4], want[0]),
         "an empty input in front of a different non-empty one");
  // a capacity one short: the first two blocks' bytes fit, the third's piece does not
  const s = await api.decompressBatchSettled([file], "gzip", { members: "bgzf", outCapacity: 603, ranges: [ranges[0]] });
  expect(s[0].status === "rejected" && s[0].reason.zmsg === "output capacity exceeded", "the capacity outcome");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
