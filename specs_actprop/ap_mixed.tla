------------------------------ MODULE ap_mixed ------------------------------
(* A safety and a liveness conjunct in one PROPERTY: [][x' >= x]_x is checked by the search, (x = 0) ~> (x = 2) on the state graph. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_mixed
variables x = 0;

fair process P = 1
begin
  s: while x < 2 do
       x := x + 1;
     end while;
end process

end algorithm *)

Both == [][x' >= x]_x /\ ((x = 0) ~> (x = 2))
=============================================================================
