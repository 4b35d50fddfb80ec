------------------------------ MODULE spin_fair ------------------------------
(* Written to show: The Spinner of spin_minus WITHOUT the `-`: WF_vars(Spinner) makes it leave the loop once the fair Setter has set the flag.  Termination HOLDS. *)
EXTENDS Naturals

(* --algorithm spin_fair
variables flag = 0, turns = 0;

fair process Spinner = 0
begin
  spin: while flag = 0 do
          turns := 1 - turns;
        end while;
end process

fair process Setter = 1
begin
  set: flag := 1;
end process

end algorithm *)

=============================================================================
